// keyed_wire.h — the keyed wire form (dsv_verify_*_keyed_wire*, include/dsv.h): serialized signatures
// (`Signature::to_bytes()` records: u, then the nonce points compressed) verified against a registered key
// set.  One decode kernel (k_keyed_wire.hip) in front of what a keyed call does anyway:
//   k_keyed_wire_decode<SCHEME>  records -> u | R_uv [| Rp_uv] | valid     (this header)
//   k_challenge                  valid enters as the hash's valid_in         (launch.h)
//   k_verify_keyed<SCHEME>                                                   (keyed.h)
// What the host units know about the kernel: its launcher and the layout of the decoded columns.
#pragma once
#include "keyed.h"

namespace dsv {

constexpr int kKeyedWireBlock = 256;

// ---- k_keyed_wire.hip --------------------------------------------------------------------------
// n records (32 B of u, then 32 B per nonce point) at sig + i * (32 + 32 * keyed_sig_points(scheme)), 16-byte
// aligned.  u[i] = the record's first 32 bytes as they lie; R_uv[i] (Rp_uv[i], double scheme only) = affine canonical u || v of the decompressed nonce
// point, k_decompress's bytes for every input; valid[i] = every nonce point of record i decodes (written
// once, never read).  One lane per point, the two points of a double item in adjacent lanes.
void launch_keyed_wire_decode(int scheme, const uint8_t* sig, size_t n, uint8_t* u, uint8_t* R_uv, uint8_t* Rp_uv,
                              uint8_t* valid, const uint32_t* ts_cancel, const uint8_t* ts_hash, hipStream_t s);

}  // namespace dsv
