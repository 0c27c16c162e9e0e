/* fd_ed25519_sign_kern.hip -- MI355X (gfx950) Ed25519 batch signing and key
   derivation: the kernels.  A second translation unit of the code object
   fd_ed25519_gpu_kern.hip builds (firedancer_amd/Makefile links both), so the
   verify kernels' code does not depend on this file.  Device functions:
   fd_ed25519_sign_dev.h.  Launched by fd_ed25519_gpu_sign_batch_dev and
   fd_ed25519_gpu_public_from_private_batch_dev (fd_ed25519_gpu_host.cpp). */

#include <hip/hip_runtime.h>

/* the other translation unit defines the round constants under their own name */
#define fd_sha512_dev_K fd_sha512_sign_K
#include "fd_ed25519_gpu_abi.h"
#include "fd_ed25519_sign_dev.h"

#define FD_SIGN_BLOCK 256

/* Public key i = encode( [a_i mod l] B ), a_i the clamped low half of
   SHA-512( prv[32 i, 32 i + 32) ): fd_ed25519_public_from_private.  prv and
   out are 4-byte aligned. */
extern "C" __global__ void __launch_bounds__( FD_SIGN_BLOCK, FD_SIGN_WAVES_PER_EU )
fd_ed25519_pubkey_kernel( sign_pubkey_args args ) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if( i >= args.n ) return;
  uint32_t const * p = args.prv + 8u*i;
  uint32_t seed[ 8 ];
#pragma unroll
  for( int j=0; j<8; j++ ) seed[j] = p[j];
  uint32_t a[ 8 ], prefix[ 8 ], w[ 8 ];
  sign_seed_expand( a, prefix, seed );
  sc_reduce256( w, a );
  ge_p3 A; sign_comb( A, w, args.ctab );
  uint32_t enc[ 8 ]; ge_tobytes( enc, A );
  uint32_t * o = args.out + 8u*i;
#pragma unroll
  for( int j=0; j<8; j++ ) o[j] = enc[j];
}

/* Signature i = R || S of message desc[i] under the private key at prv_off,
   with the caller's public key at pub_off hashed as given (not re-derived):
   fd_ed25519_sign.  A descriptor with a field outside the arena (no host has
   checked the device-resident form's) yields 64 zero bytes.  out is 4-byte
   aligned. */
extern "C" __global__ void __launch_bounds__( FD_SIGN_BLOCK, FD_SIGN_WAVES_PER_EU )
fd_ed25519_sign_kernel( sign_args args ) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if( i >= args.n ) return;
  fd_ed25519_sign_desc_t d = args.desc[ i ];
  uint32_t * o = args.out + 16u*i;
  if( (uint64_t)d.prv_off + 32u > args.arena_sz || (uint64_t)d.pub_off + 32u > args.arena_sz ||
      (uint64_t)d.msg_off + d.msg_sz > args.arena_sz ) {
#pragma unroll
    for( int j=0; j<16; j++ ) o[j] = 0u;
    return;
  }
  uint32_t const * a32 = (uint32_t const *)args.arena;
  uint32_t lim_dw = (uint32_t)((args.arena_sz + 3u) >> 2) + 1u;
  uint32_t msg_sz = d.msg_sz;

  uint32_t a[ 8 ], r[ 8 ];
  {
    uint32_t seed[ 8 ], prefix[ 8 ], dg[ 16 ];
    sign_load8( seed, a32, d.prv_off, lim_dw );
    sign_seed_expand( a, prefix, seed );
    sign_hash<8>( dg, prefix, a32, d.msg_off, msg_sz, lim_dw );
    sc_reduce512( r, dg );
  }
  uint32_t ra[ 16 ];                                   /* R || A */
  {
    ge_p3 R; sign_comb( R, r, args.ctab );
    uint32_t enc[ 8 ]; ge_tobytes( enc, R );
#pragma unroll
    for( int j=0; j<8; j++ ) ra[j] = enc[j];
  }
  {
    uint32_t pub[ 8 ];
    sign_load8( pub, a32, d.pub_off, lim_dw );
#pragma unroll
    for( int j=0; j<8; j++ ) ra[8+j] = pub[j];
  }
  uint32_t k[ 8 ], s[ 8 ];
  {
    uint32_t dg[ 16 ];
    sign_hash<16>( dg, ra, a32, d.msg_off, msg_sz, lim_dw );
    sc_reduce512( k, dg );
  }
  sc_muladd( s, k, a, r );
#pragma unroll
  for( int j=0; j<8; j++ ) { o[j] = ra[j]; o[8+j] = s[j]; }
}
