// sign_host_check.cpp -- TEST ONLY: compiles the signer's device functions
// (firedancer_amd/csrc/fd_ed25519_sign_dev.h and its additions to the
// *_dev.h headers) for the host so tests/test_sign_host.py can hold them to
// Python integers and hashlib.
#include <string.h>
#include "../../firedancer_amd/csrc/fd_ed25519_sign_dev.h"

/* [s]B in projective form with Z != 1: double-and-add over the bits of s
   (the comb table lives on the GPU only) */
static void base_mul( ge_p3 & acc, uint32_t const s[ 8 ] ) {
  uint32_t benc[ 8 ];
  benc[0] = 0x66666658u;
  for( int i=1; i<8; i++ ) benc[i] = 0x66666666u;
  ge_p3 B; ge_decode( B, benc, true );
  ge_cached Bc; ge_to_cached( Bc, B );
  ge_identity( acc );
  for( int bit=255; bit>=0; bit-- ) {
    ge_dbl( acc, acc, true );
    if( (s[bit >> 5] >> (bit & 31)) & 1u ) ge_add_cached( acc, acc, Bc, true );
  }
}

extern "C" {

void t_sc_muladd( uint32_t * s, uint32_t const * k, uint32_t const * a, uint32_t const * r ) { sc_muladd( s, k, a, r ); }
void t_sc_reduce256( uint32_t * r, uint32_t const * x ) { sc_reduce256( r, x ); }

/* x -> x mod l -> comb_bias -> the 11 signed digits */
void t_reduce_comb_digits( int * d, uint32_t const * x ) {
  uint32_t w[ 8 ], y[ 8 ];
  sc_reduce256( w, x ); comb_bias( y, w );
  for( int k=0; k<11; k++ ) d[k] = comb_digit( y, k );
}

/* encode( [s]B ); *z_is_one reports whether the projective Z was 1 */
void t_base_mul_tobytes( uint32_t * enc, uint32_t const * s, int * z_is_one ) {
  ge_p3 P; base_mul( P, s );
  uint32_t zb[ 8 ]; fe_tobytes32( zb, P.Z );
  *z_is_one = zb[0] == 1u && !(zb[1]|zb[2]|zb[3]|zb[4]|zb[5]|zb[6]|zb[7]);
  ge_tobytes( enc, P );
}

void t_seed_expand( uint32_t * a, uint32_t * prefix, uint32_t const * seed ) { sign_seed_expand( a, prefix, seed ); }

/* SHA-512( hdr || arena[msg_off, msg_off + msg_sz) ), hdr 8 or 16 words; the
   arena is readable up to dword lim_dw */
void t_sign_hash( uint32_t * dg, int hw, uint32_t const * hdr, uint32_t const * a32, uint32_t msg_off, uint32_t msg_sz,
                  uint32_t lim_dw ) {
  if( hw == 8 ) sign_hash<8>( dg, hdr, a32, msg_off, msg_sz, lim_dw );
  else          sign_hash<16>( dg, hdr, a32, msg_off, msg_sz, lim_dw );
}

/* The sign kernel's sequence on the host, [r]B by double-and-add */
void t_sign( uint32_t * sig, uint32_t const * a32, uint32_t arena_sz, uint32_t prv_off, uint32_t pub_off, uint32_t msg_off,
             uint32_t msg_sz ) {
  uint32_t lim_dw = ((arena_sz + 3u) >> 2) + 1u;
  uint32_t seed[ 8 ], a[ 8 ], prefix[ 8 ], r[ 8 ], k[ 8 ], s[ 8 ], dg[ 16 ], ra[ 16 ];
  sign_load8( seed, a32, prv_off, lim_dw );
  sign_seed_expand( a, prefix, seed );
  sign_hash<8>( dg, prefix, a32, msg_off, msg_sz, lim_dw );
  sc_reduce512( r, dg );
  ge_p3 R; base_mul( R, r );
  ge_tobytes( ra, R );
  sign_load8( ra + 8, a32, pub_off, lim_dw );
  sign_hash<16>( dg, ra, a32, msg_off, msg_sz, lim_dw );
  sc_reduce512( k, dg );
  sc_muladd( s, k, a, r );
  for( int j=0; j<8; j++ ) { sig[j] = ra[j]; sig[8+j] = s[j]; }
}

}
