// keyed_open.h — the open-set form of verify by key value (dsv_verify_keyed_open*, include/dsv.h; DESIGN.md
// §10.5): what the host unit knows about k_keyed_open.hip.  Behind the closed-set launches (lookup, challenge
// hash, keyed kernel — a miss got verdict 0 there) the items whose key the lookup did not find are listed on the
// device and decided by the unkeyed equation, in a launch sized for the whole batch whose workgroups past the
// list's end return at once: the number of misses is never known to the host.
#pragma once
#include "keyed_lookup.h"

namespace dsv {

constexpr int kMissBlock = 256;
constexpr unsigned kMaxMissGrid = 2048;

// ---- k_keyed_open.hip --------------------------------------------------------------------------
// list[0 .. *count) = the positions i < n with key_idx[i] == kSlotEmpty, in no particular order; `count`
// (one device word) is zeroed on `s` by this launcher first (launch_store_word).  `list` holds n words; one
// atomic per wave.  The launches' errors surface through hipGetLastError().
hipError_t launch_miss_list(const uint32_t* key_idx, size_t n, uint32_t* list, uint32_t* count, hipStream_t s);
// launch_verify_half (launch.h) over a list: ok[i] = valid[i] & [every chain's equation holds] for i = list[j],
// j < min(*count, n), every column read at row i; an entry >= n is skipped and ok[] is left as it is everywhere
// else.  verify_grid(n) one-wave workgroups, each reading *count once; var_tables as for launch_verify_half.
void launch_verify_listed(int nchain, const uint8_t* u, const uint8_t* c, ChainOperands op0, ChainOperands op1,
                          const uint8_t* valid, size_t n, uint8_t* ok, uint32_t* var_tables, const uint32_t* list,
                          const uint32_t* count, hipStream_t s);

// ---- k_keyed_open_var.hip ----------------------------------------------------------------------
// launch_verify_var's one-lane kernel (launch.h) over a list, the var-generator scheme's miss branch:
// ok[i] = valid[i] & [u*Gen + c*PK == R] for i = list[j], j < min(*count, n), every column read at row i; an
// entry >= n is skipped and ok[] is left as it is everywhere else.  verify_grid(n) one-wave workgroups, each
// reading *count once; var_tables: three window tables per lane, as for launch_verify_var.  No gate.
void launch_verify_var_listed(const uint8_t* u, const uint8_t* c, const uint8_t* PK_uv, const uint8_t* Gen_uv,
                              const uint8_t* R_uv, const uint8_t* valid, size_t n, uint8_t* ok,
                              uint32_t* var_tables, const uint32_t* list, const uint32_t* count, hipStream_t s);

}  // namespace dsv
