/* fd_ed25519_sign_dev.h -- the signing half of fd_ed25519.h for gfx950, one
   key or signature per lane.

   Replaces fd_ed25519_public_from_private and fd_ed25519_sign
   (src/ballet/ed25519/fd_ed25519_user.c:4-132):
     seed -> SHA-512 -> clamped scalar a, prefix          sign_seed_expand
     r = SHA-512(prefix || M) mod l                       sign_hash<8>
     R = encode([r]B): 11 mixed additions from the comb   sign_comb, ge_tobytes
     k = SHA-512(R || A || M) mod l                       sign_hash<16>
     S = (r + k a) mod l                                  sc_muladd
   The hashes keep the state and the schedule in VGPRs and stream the message
   from HBM one block ahead, as the verify kernels' hash_ram does; the header
   (prefix, or R || A) comes from registers.

   NOT constant time: the comb entries are fetched at addresses indexed by the
   digits of a mod l and of r, unlike fd_ed25519_scalar_mul_base_const_time
   (include/fd_ed25519_gpu.h says which callers that suits).  a, the prefix
   and r live in registers only; the kernels (fd_ed25519_sign_kern.hip) build
   without scratch, so nothing derived from them is written to memory.

   Everything but the comb walk also compiles for the host
   (tests/csrc/sign_host_check.cpp). */

#ifndef FD_ED25519_SIGN_DEV_H
#define FD_ED25519_SIGN_DEV_H

#include "fd_curve25519_dev.h"
#include "fd_sha512_dev.h"
#include "fd_scalar_dev.h"

#if defined(__HIPCC__)
#define FD_SIGN_FN __device__ __forceinline__
#define FD_SIGN_ALIGNBYTE( hi, lo, sh ) __builtin_amdgcn_alignbyte( (hi), (lo), (sh) )
#else
#define FD_SIGN_FN static inline
#define FD_SIGN_ALIGNBYTE( hi, lo, sh ) ((uint32_t)(((((uint64_t)(hi)) << 32) | (lo)) >> (8u*(sh))))
#endif

/* The 64-byte digest in h as 16 LE words */
FD_SIGN_FN void sign_digest_words( uint32_t dg[ 16 ], uint64_t const h[ 8 ] ) {
#pragma unroll
  for( int i=0; i<8; i++ ) { dg[2*i] = sha_bswap32( (uint32_t)(h[i] >> 32) ); dg[2*i+1] = sha_bswap32( (uint32_t)h[i] ); }
}

/* SHA-512 of the 32-byte private key (one block): a = the clamped secret
   scalar (in [2^254, 2^255), a multiple of 8), prefix = digest bytes 32..63
   (fd_ed25519_user.c:23-32, 82-87).  seed, a, prefix: 8 LE words each. */
FD_SIGN_FN void sign_seed_expand( uint32_t a[ 8 ], uint32_t prefix[ 8 ], uint32_t const seed[ 8 ] ) {
  uint64_t h[ 8 ]; sha512_init_state( h );
  uint64_t W[ 16 ];
#pragma unroll
  for( int j=0; j<4; j++ ) W[j] = ((uint64_t)sha_bswap32( seed[2*j] ) << 32) | sha_bswap32( seed[2*j+1] );
  W[4] = 0x8000000000000000ULL;
#pragma unroll
  for( int j=5; j<15; j++ ) W[j] = 0ULL;
  W[15] = 256ULL;
  sha512_compress( h, W );
  uint32_t dg[ 16 ]; sign_digest_words( dg, h );
#pragma unroll
  for( int i=0; i<8; i++ ) { a[i] = dg[i]; prefix[i] = dg[8+i]; }
  a[0] &= 0xfffffff8u;
  a[7]  = (a[7] & 0x7fffffffu) | 0x40000000u;
}

/* Raw dwords of SHA block b of header || message, the header HW words long:
   dword (msg_off >> 2) + 32 b - HW + i, i < 33, clamped to the readable arena
   [0, lim_dw] (the first HW of block 0 are not used). */
template<int HW>
FD_SIGN_FN void sign_fetch( uint32_t raw[ 33 ], uint32_t const * a32, uint32_t msg_off, uint32_t b, uint32_t lim_dw ) {
  int32_t start = (int32_t)(msg_off >> 2) + 32*(int32_t)b - HW;
#pragma unroll
  for( int i=0; i<33; i++ ) {
    int32_t x = start + i;
    uint32_t u = x < 0 ? 0u : (uint32_t)x;
    raw[i] = a32[ u < lim_dw ? u : lim_dw ];
  }
}

/* dg = SHA-512( hdr || M ) as 16 LE words; hdr: HW = 8 or 16 LE words in
   registers (32 or 64 bytes), M = arena[msg_off, msg_off + msg_sz) streamed
   through aligned dwords, each block's fetched while the previous one is
   compressed.  HW = 16 computes what hash_ram (fd_ed25519_gpu_kern.hip)
   does before its reduction. */
template<int HW>
FD_SIGN_FN void sign_hash( uint32_t dg[ 16 ], uint32_t const hdr[ HW ], uint32_t const * a32, uint32_t msg_off,
                           uint32_t msg_sz, uint32_t lim_dw ) {
  static_assert( HW == 8 || HW == 16, "a 32- or 64-byte header" );
  uint64_t h[ 8 ]; sha512_init_state( h );
  uint32_t total = 4u*HW + msg_sz;
  uint32_t nblk = (total + 17u + 127u) >> 7;
  uint32_t sh = msg_off & 3u;
  uint32_t nxt[ 33 ];
  sign_fetch<HW>( nxt, a32, msg_off, 0u, lim_dw );
  for( uint32_t b=0; b<nblk; b++ ) {
    uint32_t raw[ 33 ];
#pragma unroll
    for( int i=0; i<33; i++ ) raw[i] = nxt[i];
    if( b + 1u < nblk ) sign_fetch<HW>( nxt, a32, msg_off, b + 1u, lim_dw );
    uint64_t W[ 16 ];
#pragma unroll
    for( int j=0; j<16; j++ ) {
      uint32_t hi, lo;                                  /* big-endian halves */
      if( b == 0 && j < HW/2 ) {
        hi = sha_bswap32( hdr[2*j] ); lo = sha_bswap32( hdr[2*j+1] );
      } else {
        int32_t m = (int32_t)((b << 7) + 8u*(uint32_t)j) - 4*HW;   /* message byte index of the word's first byte */
        uint32_t w0 = FD_SIGN_ALIGNBYTE( raw[2*j+1], raw[2*j],   sh );   /* bytes m..m+3 LE */
        uint32_t w1 = FD_SIGN_ALIGNBYTE( raw[2*j+2], raw[2*j+1], sh );   /* bytes m+4..m+7  */
        hi = sha_bswap32( w0 ); lo = sha_bswap32( w1 );
        /* padding: keep bytes < msg_sz, 0x80 at msg_sz, zeros after */
        int32_t rem0 = (int32_t)msg_sz - m;             /* valid bytes from m   */
        int32_t rem1 = rem0 - 4;
        uint32_t keep0 = rem0 >= 4 ? 0xffffffffu : (rem0 <= 0 ? 0u : ~(0xffffffffu >> (8*rem0)));
        uint32_t keep1 = rem1 >= 4 ? 0xffffffffu : (rem1 <= 0 ? 0u : ~(0xffffffffu >> (8*rem1)));
        uint32_t pad0  = (rem0 >= 0 && rem0 < 4) ? (0x80000000u >> (8*rem0)) : 0u;
        uint32_t pad1  = (rem1 >= 0 && rem1 < 4) ? (0x80000000u >> (8*rem1)) : 0u;
        hi = (hi & keep0) | pad0;
        lo = (lo & keep1) | pad1;
        if( b == nblk-1u && j == 15 ) { hi = total >> 29; lo = total << 3; }
        if( b == nblk-1u && j == 14 ) { hi = 0u; lo = 0u; }
      }
      W[j] = ((uint64_t)hi << 32) | lo;
    }
    sha512_compress( h, W );
  }
  sign_digest_words( dg, h );
}

/* 8 LE words at an arbitrary byte offset of the arena, through aligned
   dwords clamped to [0, lim_dw]. */
FD_SIGN_FN void sign_load8( uint32_t out[ 8 ], uint32_t const * a32, uint32_t off, uint32_t lim_dw ) {
  uint32_t dw = off >> 2, sh = off & 3u;
  uint32_t prev = a32[ dw < lim_dw ? dw : lim_dw ];
#pragma unroll
  for( int i=0; i<8; i++ ) {
    uint32_t x = dw + 1u + (uint32_t)i;
    uint32_t nx = a32[ x < lim_dw ? x : lim_dw ];
    out[i] = FD_SIGN_ALIGNBYTE( nx, prev, sh );
    prev = nx;
  }
}

#if defined(__HIPCC__)

#include "fd_ed25519_gpu_abi.h"

/* Comb-table entry |d| of position k (fd_ed25519_gpu_abi.h FD_CTAB_*): the
   loads are issued here, the digit's sign is applied by sign_ctab_finish at
   the use point. */
FD_SIGN_FN void sign_ctab_fetch( uint32_t w[ 32 ], uint32_t const * ctab, int k, int d ) {
  uint32_t e = min( (uint32_t)(d < 0 ? -d : d), FD_CTAB_HALF );    /* |d| <= 2^22 by construction; never past the table */
  uint4 const * p = (uint4 const *)(ctab + ((uint64_t)k * FD_CTAB_N + e) * FD_CTAB_STRIDE);
#pragma unroll
  for( int j=0; j<8; j++ ) { uint4 v = p[j]; w[4*j] = v.x; w[4*j+1] = v.y; w[4*j+2] = v.z; w[4*j+3] = v.w; }
}

FD_SIGN_FN void sign_ctab_finish( ge_precomp & q, uint32_t const w[ 32 ], int d ) {
  bool neg = d < 0;
  fe t;
#pragma unroll
  for( int j=0; j<10; j++ ) t.v[j] = w[20+j];
  fe_cneg( q.T2d, t, neg );
#pragma unroll
  for( int j=0; j<10; j++ ) {
    q.YpX.v[j] = neg ? w[10+j] : w[j];
    q.YmX.v[j] = neg ? w[j]    : w[10+j];
  }
}

/* Digit k of the biased scalar y, then y >>= 23: the digits come off the
   bottom of a register-resident y (no indexed access, so no scratch). */
FD_SIGN_FN int sign_next_digit( uint32_t y[ 8 ], int k ) {
  int d = (int)(y[0] & ((1u << FD_CTAB_BITS) - 1u)) - (k < FD_CTAB_POS-1 ? (1 << (FD_CTAB_BITS-1)) : 0);
#pragma unroll
  for( int j=0; j<7; j++ ) y[j] = __builtin_amdgcn_alignbit( y[j+1], y[j], FD_CTAB_BITS );
  y[7] >>= FD_CTAB_BITS;
  return d;
}

/* c = [w]B for w < l: FD_CTAB_POS mixed additions from the identity, each
   entry fetched one addition ahead (comb_only's schedule); no doublings.
   c.T is not computed (ge_tobytes does not read it). */
FD_SIGN_FN void sign_comb( ge_p3 & c, uint32_t const w[ 8 ], uint32_t const * ctab ) {
  uint32_t y[ 8 ]; comb_bias( y, w );
  ge_identity( c );
  uint32_t craw[ 32 ];
  int d = sign_next_digit( y, 0 );
  sign_ctab_fetch( craw, ctab, 0, d );
#pragma unroll 1
  for( int k=0; k<FD_CTAB_POS; k++ ) {
    ge_precomp bp;
    sign_ctab_finish( bp, craw, d );
    if( k + 1 < FD_CTAB_POS ) { d = sign_next_digit( y, k + 1 ); sign_ctab_fetch( craw, ctab, k + 1, d ); }
    FE_FENCE();
    ge_madd( c, c, bp, k + 1 < FD_CTAB_POS );
    FE_FENCE();
  }
}

#endif /* __HIPCC__ */

#endif /* FD_ED25519_SIGN_DEV_H */
