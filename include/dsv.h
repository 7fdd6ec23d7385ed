/* dsv.h — C ABI of the MI355X batch Schnorr-verify engine (libdsv.so).
 *
 * Drop-in boundary for the native verification path of dusk-schnorr 0.18.  The reference has
 * no FFI of its own; the entry points below are what a Rust `extern "C"` block in that crate
 * would bind to offload its three verify functions (binding shown in INTEGRATION.md):
 *
 *   dsv_verify_single   replaces  PublicKey::verify        /root/reference/src/keys/public.rs:121-130
 *   dsv_verify_double   replaces  PublicKeyDouble::verify  /root/reference/src/keys/public.rs:222-244
 *   dsv_verify_vargen   replaces  PublicKeyVarGen::verify  /root/reference/src/keys/public.rs:401-415
 *   dsv_challenge_*     exposes   challenge_hash{,_double} /root/reference/src/signatures.rs:127-134, 275-290
 *   dsv_sign_*          computes what SecretKey::sign / sign_double / SecretKeyVarGen::sign compute
 *                                                          /root/reference/src/keys/secret.rs:150-168, 217-240, 433-451
 *   dsv_public_keys     computes  PublicKey::from(&SecretKey)  /root/reference/src/keys/public.rs:61-67, 265-272
 *                       — as INPUT GENERATORS for tests and benchmarks, not as a production
 *                       signer: see the note at the signing section.
 *
 * Data layout (all entry points): structure-of-arrays, caller-owned, one batch = n items.
 *   scalar  (JubJubScalar u, sk, c; BlsScalar message m) : 32 bytes, canonical little-endian
 *                                                           (what `to_bytes()` yields)
 *   point   (R, R', PK, PK', Gen)                         : 64 bytes = affine u || v, each a
 *                                                           canonical LE BlsScalar, i.e. the pair
 *                                                           `JubJubExtended::to_hash_inputs()` returns
 *   ext point (the *_ext entry points)                     : 96 bytes = u || v || z of a
 *                                                           JubJubExtended with arbitrary z != 0,
 *                                                           each coordinate canonical LE (what
 *                                                           get_u/get_v/get_z().to_bytes() yield);
 *                                                           z = 0 or a coordinate >= q: ok[i] = 0
 *   verdict ok[i]                                          : one byte, 1 = verify() true, 0 = false
 * Verdicts are those of the reference's `verify` for every input its types can hold (any
 * on-curve point incl. identity / small order, any scalar) — bit-exact against this repository's
 * CPU restatement of the reference algorithm (oracle/); the challenge hash's constants are
 * recipe-derived and NOT pinned by any upstream vector ("parity unpinned").
 * Encodings the Rust types
 * cannot hold (scalar >= r, coordinate or message >= q) give ok[i] = 0; off-curve
 * coordinates are out of contract (result unspecified, never a fault).
 *
 * Host entry points take HOST pointers (pageable is fine), stage through library-owned pinned
 * and device buffers in chunks of 2^15 .. 2^18 items (DSV_HOST_THREADS / dsv_set_host_threads copy
 * threads per call, default 4; six library-owned streams per device, the two that carry the kernels
 * on different priority levels so that they never share a hardware queue) and block until the
 * verdicts are in `ok`.  The *_dev entry points take DEVICE pointers (hipMalloc'd,
 * 16-byte aligned) plus a hipStream_t passed as void*, enqueue only, and never synchronise —
 * they are what the bench times with inputs resident in HBM.
 *
 * Devices and threads.  dsv_init(d) may be called for several devices of one process; each gets
 * its own context (tables, streams, staging) and nothing is shared between contexts.
 *   - *_dev entry points run on the device that OWNS their output buffer (the stream must belong
 *     to the same device); they may be called concurrently from any number of threads, on the
 *     same or on different streams, and leave the calling thread's current device unchanged.
 *     Callers on different streams get different internal sub-batch streams (up to 8 per device,
 *     shared beyond that), so they overlap on the GPU.
 *   - host entry points run on the calling thread's device: dsv_set_device(d) (thread-local), else
 *     the first device initialised.  Up to dsv_max_in_flight() (2) verify calls run concurrently on
 *     ONE device, each with its own staging, sharing the device's compute streams (a further call
 *     waits its turn, first come first served); host calls on different devices run in parallel.
 *     The small utility entry points (challenge, sign, decompress, debug) serialise on a lock.
 *   - dsv_verify_*_multi shard one host batch over ALL initialised devices (contiguous shards, one
 *     host thread per device, no collective).
 *   - dsv_shutdown[_device] waits for the host calls (and jobs) in flight on that device, synchronises the
 *     device and releases everything; the caller must not have *_dev work of its own still
 *     enqueued whose workspace it frees, and must not start new calls on that device until a
 *     later dsv_init.  Calls that arrive after shutdown return DSV_ERR_NOT_INITIALIZED.
 *
 * Return value: DSV_OK (0) or a negative dsv_status; dsv_last_error() gives the text for
 * the calling thread.  The library keeps no pointer after a call returns.  dsv_init is
 * idempotent and thread-safe.
 */
#ifndef DSV_H
#define DSV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DSV_OK = 0,
  DSV_ERR_NOT_INITIALIZED = -1,
  DSV_ERR_INVALID_ARGUMENT = -2,
  DSV_ERR_HIP = -3,
  DSV_ERR_NO_DEVICE = -4,
  DSV_ERR_TOO_LARGE = -5
} dsv_status;

#define DSV_MAX_BATCH ((size_t)1 << 28)

/* ---- lifecycle ---- */
int dsv_init(int device);             /* create this GPU's context: fixed-base tables for G and G'
                                         (2 x 75.5 MB, ~50 ms of device time) */
int dsv_init_visible(void);           /* dsv_init for every device listed in the environment variable
                                         DSV_DEVICES ("0,2,3"), else for every visible device;
                                         returns how many are initialised or a negative status */
int dsv_shutdown(void);               /* every initialised device */
int dsv_shutdown_device(int device);
int dsv_set_device(int device);       /* device of THIS thread's host entry points (must be initialised) */
int dsv_get_device(void);             /* ... the current choice; -1 before any dsv_init */
int dsv_initialized_devices(int *out, int cap);
/* NUMA placement (an 8-GPU host has two sockets).  dsv_init reads the device's PCI address and, from
 * /sys/bus/pci/devices/<address>/numa_node and /sys/devices/system/node/node<N>/cpulist, the cpus of the
 * socket its PCIe root hangs off; the copy threads of that device's host calls and the library's own
 * per-device worker threads (*_multi shards beyond the first, the drivers of submitted jobs) are bound to
 * them (threads of the application never are).  Pinned staging needs nothing: hipHostMalloc allocates on
 * the node nearest the current device.  DSV_NUMA=0 in the environment switches the binding off;
 * DSV_SYSFS_ROOT points the lookup at another tree.  dsv_device_numa: *node (-1: unknown), up to `cap`
 * cpus and the PCI address (bdf: NULL or >= 32 bytes) of an initialised device; returns the cpu count or a
 * negative dsv_status.  dsv_debug_numa_lookup: the lookup alone, no device needed (tests). */
int dsv_device_numa(int device, int *node, int *cpus, int cap, char *bdf);
int dsv_debug_numa_lookup(const char *sysfs_root, const char *bdf, int *node, int *cpus, int cap); /* returns how many; fills out[0 .. min(cap, count)) */
const char *dsv_version(void);
const char *dsv_last_error(void);
int dsv_device_count(void);
int dsv_set_host_threads(int n);      /* copy threads the host entry points gather the caller's arrays with
                                         (per process, 1..16): n >= 1 sets, 0 restores the default (the
                                         environment variable DSV_HOST_THREADS, else 4); returns the value
                                         in force */

/* ---- verify, host buffers ---- */
int dsv_verify_single(const uint8_t *u, const uint8_t *R_uv, const uint8_t *PK_uv,
                      const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double(const uint8_t *u, const uint8_t *R_uv, const uint8_t *Rp_uv,
                      const uint8_t *PK_uv, const uint8_t *PKp_uv, const uint8_t *m, size_t n,
                      uint8_t *ok);
int dsv_verify_vargen(const uint8_t *u, const uint8_t *R_uv, const uint8_t *PK_uv,
                      const uint8_t *Gen_uv, const uint8_t *m, size_t n, uint8_t *ok);
/* ---- verify, projective inputs ---------------------------------------------------------------
 * Every point as (u, v, z), 96 B: what the reference's in-memory types hold (`PublicKey::from(&sk)`
 * = GENERATOR_EXTENDED * sk and R = GENERATOR_EXTENDED * r are JubJubExtended with z != 1,
 * /root/reference/src/keys/public.rs:61-67, src/keys/secret.rs:159).  The device performs the
 * `to_hash_inputs` normalisation the reference's verify starts with
 * (/root/reference/src/signatures.rs:131, :280-281) — at most one field inversion per signature,
 * shared by all its points and, in large batches, by eight signatures — so the caller does no
 * field arithmetic on the host.  Same verdicts as the affine entry points on the normalised
 * points. */
int dsv_to_hash_inputs(const uint8_t *in_uvz, size_t n, uint8_t *out_uv, uint8_t *ok); /* the step alone */
int dsv_verify_single_ext(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                          const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_ext(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *Rp_uvz,
                          const uint8_t *PK_uvz, const uint8_t *PKp_uvz, const uint8_t *m, size_t n,
                          uint8_t *ok);
int dsv_verify_vargen_ext(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                          const uint8_t *Gen_uvz, const uint8_t *m, size_t n, uint8_t *ok);
/* ... sharded over every initialised device (what the Rust / C++ verify_batch* bind) */
int dsv_verify_single_ext_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                                const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_ext_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *Rp_uvz,
                                const uint8_t *PK_uvz, const uint8_t *PKp_uvz, const uint8_t *m,
                                size_t n, uint8_t *ok);
int dsv_verify_vargen_ext_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                                const uint8_t *Gen_uvz, const uint8_t *m, size_t n, uint8_t *ok);
/* ... device buffers (enqueue only); workspace: dsv_ext_workspace_bytes(n) device bytes, 256-byte
 * aligned */
size_t dsv_ext_workspace_bytes(size_t n);
int dsv_verify_single_ext_dev(const void *u, const void *R_uvz, const void *PK_uvz, const void *m,
                              size_t n, void *ok, void *workspace, void *stream);
int dsv_verify_double_ext_dev(const void *u, const void *R_uvz, const void *Rp_uvz,
                              const void *PK_uvz, const void *PKp_uvz, const void *m, size_t n,
                              void *ok, void *workspace, void *stream);
int dsv_verify_vargen_ext_dev(const void *u, const void *R_uvz, const void *PK_uvz,
                              const void *Gen_uvz, const void *m, size_t n, void *ok, void *workspace,
                              void *stream);

/* ---- verify, the reference's IN-MEMORY representation (Montgomery limbs) -----------------------
 * The Rust types hold every field element as `[u64; 4]` little-endian limbs in Montgomery form,
 * R = 2^256: `BlsScalar(pub [u64; 4])` (dusk-bls12_381 0.13), `JubJubScalar` and the coordinates
 * of `JubJubExtended` (dusk-jubjub 0.14) — /root/reference/Cargo.toml:25-26; the fields that verify
 * reads: /root/reference/src/signatures.rs:58-61, 180-184, 337-340 (u, R, R'),
 * src/keys/public.rs:59, 189, 331-334 (pk, pk', generator), the `BlsScalar` message of
 * src/keys/public.rs:121, 222-226, 401-405.  Every `to_bytes()` is a Montgomery reduction on the
 * host (8 per single signature, 14 per double one).  These entry points take the limbs as they
 * lie in memory, so a binding copies bytes and does no arithmetic at all:
 *   scalar (u, m)              : 32 B = the four u64 limbs of x * 2^256 mod (r | q)
 *   point  (R, R', PK, PK', Gen): 96 B = limbs of u || v || z of the JubJubExtended (t1, t2 are not
 *                                read; a common factor of the three coordinates does not change
 *                                the point, so the device normalises them exactly like *_ext input)
 * Limbs that are not below their modulus (the Rust types cannot hold them) or z = 0: ok[i] = 0.
 * Same verdicts as dsv_verify_*_ext on the `to_bytes()` of the same values.
 *
 * The *_mont_cols forms read the typed objects WHERE THEY LIE: one dsv_column per field, item i at
 * base + i * stride (stride = sizeof of the struct the field lives in).  The pipeline's copy threads
 * gather the fields straight into pinned staging while the GPU works on the previous chunk — no
 * intermediate structure of arrays, no second pass over host memory.  Column order:
 *   single: u, R, PK, m            double: u, R, R', PK, PK', m            vargen: u, R, PK, Gen, m
 * They shard over every initialised device like the *_multi forms (what verify_batch* bind). */
typedef struct dsv_column {
  const void *base;   /* field of item 0 */
  size_t stride;      /* bytes from one item's field to the next (>= the field's width) */
} dsv_column;
int dsv_verify_single_mont_cols(const dsv_column *cols /*[4]*/, size_t n, uint8_t *ok);
int dsv_verify_double_mont_cols(const dsv_column *cols /*[6]*/, size_t n, uint8_t *ok);
int dsv_verify_vargen_mont_cols(const dsv_column *cols /*[5]*/, size_t n, uint8_t *ok);
/* ... asynchronous: `submit` validates the arguments, hands the batch to a library-owned driver
 * thread and returns at once with a job; `dsv_job_wait` blocks until the verdicts are in `ok`, returns
 * the status the blocking form would have returned (dsv_last_error() then holds its text) and
 * releases the job — every submitted job must be waited for exactly once.  cols[] is copied; the
 * objects the columns point into and `ok` must stay valid until the wait returns.
 * Why: a single call pays a ramp (the GPU idles until the first chunk has been gathered and
 * transferred, then runs small first chunks at low occupancy) and a tail.  With two batches in
 * flight the second one's ramp runs under the first one's tail: each call in flight owns its own
 * staging (dsv_max_in_flight() per device; a further job waits inside its driver thread), the
 * compute streams are shared, so the GPU sees one queue of sub-batches.  The blocking host entry
 * points may equally be called from several threads at once — same mechanism.
 * Jobs start in submission order.  dsv_job_done: 1 finished / 0 running (does not release).
 * dsv_shutdown* first lets every job submitted so far (and every blocking call that already owns
 * its staging) run to its verdicts; a submit racing with the shutdown may fail with
 * DSV_ERR_NOT_INITIALIZED at its wait. */
/* ... with the batch fast accept (dsv_verify_*_rlc_dev below: same verdicts; ONE aggregate test decides
 * "all true", anything else is decided by the per-signature kernels): the pipeline only fills a
 * per-device arena — gather, transfer, normalisation and the challenge hash chunk by chunk while the
 * transfers run — then the aggregate runs over the resident group.  With several devices initialised
 * and >= 2^17 items per device the batch is sharded like the *_multi forms, one group (one aggregate)
 * per device; else one group (2^17 <= n <= 2^22) on the calling thread's device; larger and smaller
 * batches take the ordinary column path.  One such call at a time per device.  *accepted (may be NULL): 1 = every
 * group's aggregate decided. */
int dsv_verify_single_mont_cols_rlc(const dsv_column *cols /*[4]*/, size_t n, uint8_t *ok, int *accepted);
int dsv_verify_double_mont_cols_rlc(const dsv_column *cols /*[6]*/, size_t n, uint8_t *ok, int *accepted);
int dsv_verify_vargen_mont_cols_rlc(const dsv_column *cols /*[5]*/, size_t n, uint8_t *ok, int *accepted);
typedef struct dsv_job dsv_job;
int dsv_verify_single_mont_cols_submit(const dsv_column *cols /*[4]*/, size_t n, uint8_t *ok, dsv_job **job);
int dsv_verify_double_mont_cols_submit(const dsv_column *cols /*[6]*/, size_t n, uint8_t *ok, dsv_job **job);
int dsv_verify_vargen_mont_cols_submit(const dsv_column *cols /*[5]*/, size_t n, uint8_t *ok, dsv_job **job);
int dsv_job_wait(dsv_job *job);
int dsv_job_done(const dsv_job *job);
int dsv_max_in_flight(void);
/* ... dense arrays (structure of arrays), this thread's device */
int dsv_verify_single_mont(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                           const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_mont(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *Rp_uvz,
                           const uint8_t *PK_uvz, const uint8_t *PKp_uvz, const uint8_t *m, size_t n,
                           uint8_t *ok);
int dsv_verify_vargen_mont(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                           const uint8_t *Gen_uvz, const uint8_t *m, size_t n, uint8_t *ok);
/* ... dense arrays, sharded over every initialised device */
int dsv_verify_single_mont_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                                 const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_mont_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *Rp_uvz,
                                 const uint8_t *PK_uvz, const uint8_t *PKp_uvz, const uint8_t *m,
                                 size_t n, uint8_t *ok);
int dsv_verify_vargen_mont_multi(const uint8_t *u, const uint8_t *R_uvz, const uint8_t *PK_uvz,
                                 const uint8_t *Gen_uvz, const uint8_t *m, size_t n, uint8_t *ok);
/* ... device buffers (enqueue only); workspace: dsv_mont_workspace_bytes(n) device bytes, 256-byte
 * aligned */
size_t dsv_mont_workspace_bytes(size_t n);
int dsv_verify_single_mont_dev(const void *u, const void *R_uvz, const void *PK_uvz, const void *m,
                               size_t n, void *ok, void *workspace, void *stream);
int dsv_verify_double_mont_dev(const void *u, const void *R_uvz, const void *Rp_uvz,
                               const void *PK_uvz, const void *PKp_uvz, const void *m, size_t n,
                               void *ok, void *workspace, void *stream);
int dsv_verify_vargen_mont_dev(const void *u, const void *R_uvz, const void *PK_uvz,
                               const void *Gen_uvz, const void *m, size_t n, void *ok, void *workspace,
                               void *stream);

/* ---- verify, host buffers, sharded over every initialised device (see "Devices and threads") ---- */
int dsv_verify_single_multi(const uint8_t *u, const uint8_t *R_uv, const uint8_t *PK_uv,
                            const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_multi(const uint8_t *u, const uint8_t *R_uv, const uint8_t *Rp_uv,
                            const uint8_t *PK_uv, const uint8_t *PKp_uv, const uint8_t *m,
                            size_t n, uint8_t *ok);
int dsv_verify_vargen_multi(const uint8_t *u, const uint8_t *R_uv, const uint8_t *PK_uv,
                            const uint8_t *Gen_uv, const uint8_t *m, size_t n, uint8_t *ok);

/* ---- verify, device buffers (enqueue only) ----
 * workspace: device scratch of dsv_workspace_bytes(n) bytes, 256-byte aligned, owned by the call
 * until its work on `stream` has completed (two calls in flight need two workspaces).
 * Ordering: everything the call enqueues happens after the work already on `stream` and before
 * anything enqueued on `stream` afterwards.  Batches of >= 2^17 items are cut into 2^16-item
 * parts that run on two library-owned streams forked from / joined to `stream` by events
 * (DSV_SPLIT=0 in the environment at dsv_init keeps every launch on `stream` itself).  Batches of
 * <= 2^14 items run an eight-lanes-per-signature kernel that trades throughput for latency, with
 * their window tables built on a library-owned stream beside the hash (DSV_QUAD=0 keeps them on
 * the one-lane kernel, DSV_SMALL_OVERLAP=0 builds the tables inside the verify kernel).  Same verdicts on every path. */
size_t dsv_workspace_bytes(size_t n);
int dsv_verify_single_dev(const void *u, const void *R_uv, const void *PK_uv, const void *m,
                          size_t n, void *ok, void *workspace, void *stream);
int dsv_verify_double_dev(const void *u, const void *R_uv, const void *Rp_uv, const void *PK_uv,
                          const void *PKp_uv, const void *m, size_t n, void *ok, void *workspace,
                          void *stream);
int dsv_verify_vargen_dev(const void *u, const void *R_uv, const void *PK_uv, const void *Gen_uv,
                          const void *m, size_t n, void *ok, void *workspace, void *stream);

/* ---- optional fast accept: random-linear-combination batch verification ----
 * Same inputs and the same verdict vector as dsv_verify_single_dev — what differs is the time.  Per
 * group of up to 2^22 items the call first runs ONE aggregate test (schnorr_amd/csrc/k_rlc.hip):
 *   every PK_i and R_i lies in the prime-order subgroup, and
 *   (sum z_i u_i) G + sum (z_i c_i) PK_i - sum z_i R_i == O   for secret 128-bit z_i drawn per call
 * (getrandom).  If it holds, every well-formed item's verdict is `true`, exactly as
 * `PublicKey::verify` (/root/reference/src/keys/public.rs:121-130) would say one by one — up to an
 * error probability <= 2^-112 of accepting a batch that holds a wrong signature, where the
 * per-signature path has none.  If it does not hold (one wrong signature, one point with a
 * small-order component — the reference's types can hold those and its equation is cofactorless —
 * or a point off the curve), the group is verified by dsv_verify_single_dev's kernels and gets their
 * verdicts: nothing is ever decided by the aggregate except "all true".  Worth it where batches are
 * expected to be entirely valid (~2.7x less arithmetic then).
 * ENQUEUE-ONLY like every other *_dev call: the per-signature kernels are launched unconditionally
 * behind the aggregate and return in their first instructions where it accepted (they read its flag
 * words from device memory); no decision is taken on the host.
 * Failure localisation.  A rejected group costs both paths, so the library adapts per device: a counter
 * kept by the device itself (8 after a call that held a rejected aggregate, one less after a call whose
 * aggregates all accepted, 1 after dsv_init; the host reads it without waiting, possibly one call late)
 * decides how the NEXT calls run.  While it is > 0 a group is cut into up to 16 sub-groups of >= 2^16 items
 * that share the hash and one set of launches, each with its own aggregate — one wrong signature in 2^20
 * then sends 2^16 items to the per-signature kernels, not 2^20 —, and 1024 consecutive items at a position
 * drawn from the call's secret key are verified first: a wrong one among them skips the aggregates
 * altogether (a batch tampered with throughout pays hash + sample + per-signature path; a heuristic,
 * DSV_RLC_SAMPLE=0 switches it off, DSV_RLC_SUB_LOG2 / DSV_RLC_SUBGROUPS tune / force the sub-groups).
 * A caller whose batches are valid runs one aggregate per group and nothing else.
 * window_bits: 0 = chosen from n — and groups below 2^17 items (single signatures; double and
 * var-generator batches: below 2^14), where an aggregate does not pay, go straight to the per-signature
 * kernels —, else one of 4, 6, 8, 12, 14, 16 (bucket windows; tests).
 * accepted (may be NULL): receives 1 if every group was decided by its aggregates, else 0.  If it points
 * to memory the device can write — device memory, or host memory from hipHostMalloc / hipHostRegister —
 * it is written by a kernel when `stream` gets there and the call does not block; if it is ordinary
 * host memory the call waits for `stream` at its end and stores the value itself.
 * workspace: dsv_rlc_workspace_bytes(n, window_bits) device bytes, 256-byte aligned (never less for a
 * larger n: a workspace sized for n serves any smaller batch).
 * No graph capture: the 32-byte weight key is drawn on the host (getrandom) per call and passed by value —
 * a replayed graph would reuse it, and predictable weights void the soundness of the aggregate.  So every
 * device-pointer fast accept (dsv_verify_*_rlc_dev, dsv_verify_*_wire_rlc_dev, dsv_verify_mixed_rlc_dev,
 * dsv_verify_*_keyed_rlc_dev) returns DSV_ERR_INVALID_ARGUMENT on a capturing stream before it touches the
 * stream or `accepted`.  The per-signature entry points have no such state and may be captured. */
size_t dsv_rlc_workspace_bytes(size_t n, int window_bits);
/* geometry of one group's aggregate (tests, sizing; works without a GPU): scheme 0 single / 1 double /
 * 2 var-generator, `groups` sub-groups (0 or 1: one); out[24] = window bits c, c/2, key windows, nonce
 * windows, windows, row/column segments, bit-sum segments, low digit bits sorted through LDS, multiples
 * of r added to a key scalar, long / short points and fixed-base terms per item, (digit, point) pairs
 * per sub-group, buckets per sub-group, points of the two scratch areas, high digit bits (bins per
 * window = 2^that), digit rows, digits per row, bins, slots per bin, sub-groups, items per sub-group,
 * workspace bytes of this plan */
int dsv_rlc_plan_info(int scheme, size_t n, int window_bits, int groups, uint64_t *out /*[24]*/);
/* the device's history counter (see above; tests and tools): returns it, or a negative dsv_status;
 * set >= 0 overrides it */
int dsv_debug_rlc_history(int device, int set);
/* the device's LONG history counter (128 after a call that held a rejected aggregate, one less after a call
 * whose aggregates all accepted): while it is > 0 and the short one is 0, groups run "guarded" — one aggregate
 * as in the steady state plus, behind it, a second stage of sub-group aggregates that a kernel switches off
 * when the first accepted (+0.03 ms on an accepted 2^20-item call), so that the first rejected batch after a run of valid
 * ones is localised too instead of paying both paths in full.  DSV_RLC_GUARD=0 switches that off. */
int dsv_debug_rlc_history_long(int device, int set);
/* sub-groups per group, process-wide: groups >= 1 forces that many (whatever the history says),
 * 0 = automatic, < 0 = leave; returns the previous setting ($DSV_RLC_SUBGROUPS initialises it) */
int dsv_debug_rlc_subgroups(int groups);
int dsv_verify_single_rlc_dev(const void *u, const void *R_uv, const void *PK_uv, const void *m,
                              size_t n, void *ok, void *workspace, void *stream, int window_bits,
                              int *accepted);
/* the same in front of dsv_verify_double_dev (`PublicKeyDouble::verify`, src/keys/public.rs:222-244:
 * both equations of an item enter the sum, each with a weight of its own) and of
 * dsv_verify_vargen_dev (`PublicKeyVarGen::verify`, :401-415: the generator is a third variable
 * point, its scalar z_i u_i) */
int dsv_verify_double_rlc_dev(const void *u, const void *R_uv, const void *Rp_uv, const void *PK_uv,
                              const void *PKp_uv, const void *m, size_t n, void *ok, void *workspace,
                              void *stream, int window_bits, int *accepted);
int dsv_verify_vargen_rlc_dev(const void *u, const void *R_uv, const void *PK_uv, const void *Gen_uv,
                              const void *m, size_t n, void *ok, void *workspace, void *stream,
                              int window_bits, int *accepted);

/* ... and in front of dsv_verify_*_wire_dev (serialized records resident in HBM; layouts below): decode,
 * then the aggregate.  A record that does not decode has verdict 0 and stays out of the sum; decoded
 * points lie on the curve but not necessarily in the prime-order subgroup (`from_bytes`,
 * src/keys/public.rs:94-100), which is what the aggregate's subgroup test is for.
 * workspace: dsv_wire_rlc_workspace_bytes(n, window_bits). */
size_t dsv_wire_rlc_workspace_bytes(size_t n, int window_bits);
int dsv_verify_single_wire_rlc_dev(const void *sig64, const void *pk32, const void *m, size_t n, void *ok,
                                   void *workspace, void *stream, int window_bits, int *accepted);
int dsv_verify_double_wire_rlc_dev(const void *sig96, const void *pk64, const void *m, size_t n, void *ok,
                                   void *workspace, void *stream, int window_bits, int *accepted);
int dsv_verify_vargen_wire_rlc_dev(const void *sig64, const void *pk64, const void *m, size_t n, void *ok,
                                   void *workspace, void *stream, int window_bits, int *accepted);

/* ... and from serialized records in HOST memory (the layouts of dsv_verify_*_wire): the pipeline decodes
 * chunk by chunk into a per-device arena while the transfers run (128 B per single signature on the bus,
 * half of the typed-object form), one aggregate follows.  One group, 2^17 <= n <= 2^22, on the calling
 * thread's device; other sizes take dsv_verify_*_wire. */
int dsv_verify_single_wire_rlc(const uint8_t *sig64, const uint8_t *pk32, const uint8_t *m, size_t n, uint8_t *ok,
                               int *accepted);
int dsv_verify_double_wire_rlc(const uint8_t *sig96, const uint8_t *pk64, const uint8_t *m, size_t n, uint8_t *ok,
                               int *accepted);
int dsv_verify_vargen_wire_rlc(const uint8_t *sig64, const uint8_t *pk64, const uint8_t *m, size_t n, uint8_t *ok,
                               int *accepted);

/* second stage alone: ok[i] = (accumulate ? ok[i] : valid[i]) & [u*Gen + c*PK == R], Gen = G
 * (which = 0) or G' (which = 1); c and valid as produced by dsv_challenge_*_dev */
int dsv_verify_core_dev(const void *u, const void *c, const void *valid, const void *PK_uv,
                        const void *R_uv, int which, int accumulate, size_t n, void *ok,
                        void *workspace, void *stream);

/* both equations of PublicKeyDouble::verify from a precomputed challenge, ONE launch (what
 * dsv_verify_double_dev runs after k_challenge): ok[i] = valid[i] & [uG + cPK == R] & [uG' + cPK' == R'] */
int dsv_verify_core_double_dev(const void *u, const void *c, const void *valid, const void *PK_uv,
                               const void *R_uv, const void *PKp_uv, const void *Rp_uv, size_t n,
                               void *ok, void *workspace, void *stream);

/* ---- mixed batches (single and double signatures interleaved), device buffers ----------------
 * kinds[i] = 0: item i is a Signature / PublicKey pair, 1: a SignatureDouble / PublicKeyDouble
 * pair; the batch is a structure of arrays over ALL n items (Rp_uv / PKp_uv rows of single items
 * are ignored).  The library splits the batch by kind ON THE DEVICE (stable compaction of the
 * index vector + row gathers), runs each kind through its own kernels and scatters the verdicts
 * back into batch order.  n_double = number of kind-1 items; every other item must be kind 0.  If
 * the counts do not match the kind vector, or an item has another kind, the affected verdicts
 * (all of them for a count mismatch) are 0.  kinds must be 16-byte aligned.
 * workspace: dsv_mixed_workspace_bytes(n) device bytes, 256-byte aligned. */
size_t dsv_mixed_workspace_bytes(size_t n);
int dsv_verify_mixed_dev(const void *kinds, const void *u, const void *R_uv, const void *Rp_uv,
                         const void *PK_uv, const void *PKp_uv, const void *m, size_t n,
                         size_t n_double, void *ok, void *workspace, void *stream);
/* ... with each kind's items through the batch fast accept (dsv_verify_*_rlc_dev above: same verdicts;
 * `accepted` as there: 1 = every group of both kinds was decided by its aggregates).
 * workspace: dsv_mixed_rlc_workspace_bytes(n). */
size_t dsv_mixed_rlc_workspace_bytes(size_t n);
int dsv_verify_mixed_rlc_dev(const void *kinds, const void *u, const void *R_uv, const void *Rp_uv,
                             const void *PK_uv, const void *PKp_uv, const void *m, size_t n,
                             size_t n_double, void *ok, void *workspace, void *stream, int *accepted);
/* the pieces, for callers that shard each kind separately (schnorr_amd/distributed.py):
 *   split : idx_single[j] / idx_double[j] = batch position (uint32) of the j-th item of that kind,
 *           at most cap_* entries written; scratch: dsv_split_scratch_bytes(n) device bytes whose
 *           last two uint32 (at offset dsv_split_scratch_bytes(n) - 256) receive the two counts
 *   gather: dst row j = src row idx[j], rows of row_bytes (multiple of 16) bytes, src has src_rows rows
 *   scatter: dst[idx[j]] = src[j] (verdict bytes back into batch order), dst has dst_len bytes
 *   Both touch entries j < min(count, *count_limit) only (count_limit: device uint32, e.g. one of
 *   the split's two counts; NULL = no limit) and skip an index that is out of range, so an index
 *   vector is never dereferenced beyond what the split wrote into it. */
size_t dsv_split_scratch_bytes(size_t n);
int dsv_split_kinds_dev(const void *kinds, size_t n, void *idx_single, size_t cap_single,
                        void *idx_double, size_t cap_double, void *scratch, void *stream);
int dsv_gather_rows_dev(const void *src, size_t src_rows, size_t row_bytes, const void *idx,
                        size_t count, const void *count_limit, void *dst, void *stream);
int dsv_scatter_verdicts_dev(const void *src, const void *idx, size_t count, const void *count_limit,
                             void *dst, size_t dst_len, void *stream);

/* ---- challenge hash only (c = trunc250(Poseidon(R.., m))), 32 B LE per item ---- */
int dsv_challenge_single(const uint8_t *R_uv, const uint8_t *m, size_t n, uint8_t *c);
int dsv_challenge_double(const uint8_t *R_uv, const uint8_t *Rp_uv, const uint8_t *m, size_t n,
                         uint8_t *c);
int dsv_challenge_single_dev(const void *R_uv, const void *m, size_t n, void *c, void *valid,
                             void *stream);
int dsv_challenge_double_dev(const void *R_uv, const void *Rp_uv, const void *m, size_t n,
                             void *c, void *valid, void *stream);

/* ---- signing / key derivation: input generation for tests and benchmarks ("next" row f-1) ----
 * sk, m, r canonical 32 B.  r is the caller-drawn nonce (the reference draws it from its RNG
 * inside sign()).  Outputs: u (32 B), R_uv / Rp_uv (64 B).  gen_uv == NULL means the standard
 * generator G;  for the var-generator scheme pass the per-key generator (variable base).
 * NOT A PRODUCTION SIGNER: unlike dusk-jubjub's constant-time multiplication, these kernels index
 * global-memory tables with digits of sk and of the nonce (memory addresses depend on secrets), and
 * they normalise r*G / sk*G with a VARIABLE-TIME inversion of the projective z (extended Euclid,
 * inv29.h: its step count, and whether it falls back to Fermat, depend on z — a value derived from
 * the secret scalar; projective coordinates are known to leak scalar bits).
 * The host entry points zero their device staging of sk / nonce before returning (and the
 * library zeroes staging it releases); the *_dev forms work in the caller's buffers only.
 * A scalar that is not canonical (>= r): host entry points return DSV_ERR_INVALID_ARGUMENT; the
 * *_dev forms write 0xff..ff (never a valid encoding) to that item's outputs. */
int dsv_sign_single(const uint8_t *sk, const uint8_t *m, const uint8_t *r, size_t n, uint8_t *u,
                    uint8_t *R_uv);
int dsv_sign_double(const uint8_t *sk, const uint8_t *m, const uint8_t *r, size_t n, uint8_t *u,
                    uint8_t *R_uv, uint8_t *Rp_uv);
int dsv_sign_vargen(const uint8_t *sk, const uint8_t *Gen_uv, const uint8_t *m, const uint8_t *r,
                    size_t n, uint8_t *u, uint8_t *R_uv);
/* PK = sk * G (which = 0), sk * G' (which = 1); or sk * Gen when gen_uv != NULL */
int dsv_public_keys(const uint8_t *sk, int which, const uint8_t *gen_uv, size_t n,
                    uint8_t *PK_uv);
int dsv_sign_single_dev(const void *sk, const void *m, const void *r, size_t n, void *u,
                        void *R_uv, void *stream);
int dsv_sign_double_dev(const void *sk, const void *m, const void *r, size_t n, void *u,
                        void *R_uv, void *Rp_uv, void *stream);
int dsv_public_keys_dev(const void *sk, int which, size_t n, void *PK_uv, void *stream);
/* variable-base forms (var-generator scheme); workspace: dsv_workspace_bytes(n) device bytes */
int dsv_public_keys_vargen_dev(const void *sk, const void *Gen_uv, size_t n, void *PK_uv,
                               void *workspace, void *stream);
int dsv_sign_vargen_dev(const void *sk, const void *Gen_uv, const void *m, const void *r, size_t n,
                        void *u, void *R_uv, void *workspace, void *stream);

/* ---- wire formats (the reference's Serializable impls) ------------------------------------
 * compressed point = JubJubAffine::to_bytes(): canonical v with bit 255 = lowest bit of u.
 * dsv_decompress_points: JubJubAffine::from_bytes for n points; ok[i] = 0 where the reference
 * would return Err (v >= q, or no square root).  The _dev form reads one 32-byte record every
 * in_stride bytes (16-byte aligned) and, with accumulate != 0, ANDs into ok[] instead of
 * overwriting it. */
int dsv_compress_points(const uint8_t *in_uv, size_t n, uint8_t *out32); /* JubJubAffine::to_bytes */
int dsv_decompress_points(const uint8_t *in32, size_t n, uint8_t *out_uv, uint8_t *ok);
int dsv_decompress_points_dev(const void *in, size_t in_stride, size_t n, void *out_uv, void *ok,
                              int accumulate, void *stream);
/* verify straight from serialized values (host buffers, array-of-records as the Rust
 * `to_bytes()` produce them):
 *   single : Signature (64 B = u || compressed R)            PublicKey (32 B)
 *            /root/reference/src/signatures.rs:106-123, src/keys/public.rs:87-101
 *   double : SignatureDouble (96 B = u || R || R')           PublicKeyDouble (64 B = pk || pk')
 *            /root/reference/src/signatures.rs:245-270, src/keys/public.rs:282-299
 *   vargen : SignatureVarGen (64 B)                          PublicKeyVarGen (64 B = pk || generator)
 *            /root/reference/src/signatures.rs:387-404, src/keys/public.rs:347-372
 * ok[i] = 1 iff every from_bytes would succeed AND verify() would return true. */
int dsv_verify_single_wire(const uint8_t *sig64, const uint8_t *pk32, const uint8_t *m, size_t n,
                           uint8_t *ok);
int dsv_verify_double_wire(const uint8_t *sig96, const uint8_t *pk64, const uint8_t *m, size_t n,
                           uint8_t *ok);
int dsv_verify_vargen_wire(const uint8_t *sig64, const uint8_t *pk64, const uint8_t *m, size_t n,
                           uint8_t *ok);
/* the same with the serialized records already in device memory (16-byte aligned; enqueue only);
 * workspace: dsv_wire_workspace_bytes(n) device bytes, 256-byte aligned */
size_t dsv_wire_workspace_bytes(size_t n);
int dsv_verify_single_wire_dev(const void *sig64, const void *pk32, const void *m, size_t n, void *ok,
                               void *workspace, void *stream);
int dsv_verify_double_wire_dev(const void *sig96, const void *pk64, const void *m, size_t n, void *ok,
                               void *workspace, void *stream);
int dsv_verify_vargen_wire_dev(const void *sig64, const void *pk64, const void *m, size_t n, void *ok,
                               void *workspace, void *stream);

/* ---- the reference harness's input generator (rand 0.8 StdRng::seed_from_u64(seed) = ChaCha12,
 * draw order per item: sk = JubJubScalar::random, m = BlsScalar::random, nonce r =
 * JubJubScalar::random; /root/reference/tests/schnorr.rs:16-22, benches/signature.rs:48-60).
 * Items first_item .. first_item + n - 1 of that stream; 32 B canonical each. */
int dsv_stdrng_sign_inputs(uint64_t seed, size_t first_item, size_t n, uint8_t *sk, uint8_t *m,
                           uint8_t *r);
int dsv_stdrng_sign_inputs_dev(uint64_t seed, size_t first_item, size_t n, void *sk, void *m,
                               void *r, void *stream);
/* var-generator harness: SecretKeyVarGen::random draws sk, then the generator scalar g
 * (Gen = g*G), then the message, then the nonce — four draws per item
 * (/root/reference/src/keys/secret.rs:371-373, tests/schnorr_var_generator.rs:16-22) */
int dsv_stdrng_vargen_inputs_dev(uint64_t seed, size_t first_item, size_t n, void *sk, void *g,
                                 void *m, void *r, void *stream);

/* ---- registered key sets: verify by key index ------------------------------------------------
 * Many messages signed under few keys (validators, committees, busy accounts): each registered key gets
 * fixed-base window tables of its points, so c*PK (and, var-generator scheme, u*Gen) become table
 * additions with no doubling: u*Gen + c*PK == R is evaluated as written.
 * scheme: 0 single (key = PK), 1 double (PK, PK'), 2 var-generator (PK, Gen); dsv_keyset_bytes(scheme, k)
 * device bytes per set (594 432 B per point and key; no GPU needed; 0 for an unknown scheme).
 *   create      : host arrays of k affine points (64 B each): pk_uv = PK, pk2_uv = PK' / Gen (NULL for
 *                 single); blocks until the tables are built.
 *   create_wire : pk_bytes = the reference's key records (PublicKey 32 B, PublicKeyDouble / PublicKeyVarGen
 *                 64 B), decoded by the device decoder of the *_wire entry points (same accepted encodings).
 * Contract:
 *   Ownership   a key set belongs to the device that was current when it was created (it must be
 *               initialised).  Its device memory is allocated once and never moves; any number of concurrent
 *               calls may read it.  It changes in two ways only: dsv_keyset_append registers further keys behind
 *               the ones it holds ("key sets that grow", below), and dsv_keyset_replace puts new keys in the places
 *               of registered ones while nothing reads the set ("keys replaced in place", below).  A call sees the
 *               set as it was when the call was enqueued; a captured graph keeps the k of its capture.
 *   Verdicts    ok[i] equals the unkeyed entry point's verdict on (u, R, PK[key_idx[i]], m) for every input
 *               the reference's types can hold.
 *   Key indices key_idx is uint32 per item; an index >= k gives ok = 0 and never a fault.
 *   Invalid keys a key with a coordinate >= q, a point off the curve, or (wire form) an encoding from_bytes
 *               rejects is recorded as invalid (dsv_keyset_key_ok: 0); every item under it gets ok = 0.
 *   Workspace   the _dev calls take workspace_bytes >= dsv_keyed_workspace_bytes(n) (device, 256-byte
 *               aligned); a shorter one returns DSV_ERR_INVALID_ARGUMENT and launches nothing.
 *   Arguments   a scheme mismatch, a key set used on another device (the owner of `ok`), or a NULL pointer
 *               with n > 0 returns DSV_ERR_INVALID_ARGUMENT; n = 0 returns DSV_OK.
 *   Enqueue-only the _dev calls never synchronise and order on `stream` like every other _dev entry point
 *               (the challenge hash, then the keyed kernel).
 *   Host forms  take host arrays, stage in chunks on the key set's device and block.
 *   Shutdown    dsv_shutdown[_device] frees the device memory of the live key sets of that device and marks
 *               them dead: verify on a dead set returns DSV_ERR_NOT_INITIALIZED, dsv_keyset_destroy releases
 *               the handle and returns DSV_OK.  dsv_keyset_destroy waits for the device's work first. */
typedef struct dsv_keyset dsv_keyset;
size_t dsv_keyset_bytes(int scheme, size_t k);
int dsv_keyset_create(int scheme, const uint8_t *pk_uv, const uint8_t *pk2_uv, size_t k, dsv_keyset **out);
int dsv_keyset_create_wire(int scheme, const uint8_t *pk_bytes, size_t k, dsv_keyset **out);
int dsv_keyset_destroy(dsv_keyset *ks);
int dsv_keyset_info(const dsv_keyset *ks, int *scheme, size_t *k, size_t *bytes, int *device);
/* key_ok: one byte per registered key.  dsv_keyset_key_ok writes k bytes, k as the call finds it: right for a set
 * that nobody appends to meanwhile.  For a set that may grow between the caller's reading of k and this call use
 * dsv_keyset_key_ok_n: it writes the first min(k, room) bytes, never more than `room`, and reports in *k_out (may
 * be NULL) the k those bytes belong to — size `out` by the set's capacity, which never changes. */
int dsv_keyset_key_ok(const dsv_keyset *ks, uint8_t *out /* k bytes */);
int dsv_keyset_key_ok_n(const dsv_keyset *ks, uint8_t *out /* room bytes */, size_t room, size_t *k_out);
/* ---- key sets that grow: reserved capacity, keys appended to a live set ---------------
 * The admission half of the key cache (dsv_verify_keyed_open*): when a new key turns busy it is registered in
 * place, at the cost of its own table, instead of a second set over all k + 1 keys.
 *   create_reserved  dsv_keyset_create with room for `capacity` >= k keys: both device allocations (the tables
 *               with key_ok, the index) are made for `capacity` keys — dsv_keyset_bytes(scheme, capacity) and
 *               dsv_keyset_index_bytes(scheme, capacity); dsv_keyset_info's `bytes` reports the former; the index
 *               has the slots of a set of `capacity` keys (dsv_debug_keyset_home_slot(scheme, capacity, ...)).
 *               k may be 0 (the key pointers may then be NULL).  Checks in this order: NULL `out`, unknown scheme
 *               (DSV_ERR_INVALID_ARGUMENT), capacity < k (DSV_ERR_INVALID_ARGUMENT), capacity > 2^32 - 2
 *               (DSV_ERR_TOO_LARGE: indices are 32-bit and DSV_KEY_NONE is taken), then those of dsv_keyset_create.
 *               The three plain constructors build sets with capacity == k.
 *   append      m more keys in the constructor's form (append: affine host bytes; append_wire: key records;
 *               append_mont_cols: `PublicKey*` objects), validated and recorded as at creation (an undecodable
 *               or invalid key gets key_ok = 0 and takes an index all the same).  On DSV_OK they have the indices
 *               *first_index .. *first_index + m - 1, *first_index = the k before the call (first_index may be
 *               NULL), and dsv_keyset_info reports k + m.  Builds the tables of the new keys only and inserts them
 *               into the index that is there: no registered key moves, an index handed out earlier stays valid, a
 *               key that was registered already (or is given twice) still looks up to its lowest index.  Blocks;
 *               runs on a stream of its own on the set's device, whatever device is current.  Once it has
 *               returned, every keyed call enqueued afterwards, on any stream of the set's device, sees the new
 *               keys.  Appends to one set are serialised; verify calls on the set go on beside an append.
 *   Errors      NULL handle, or NULL keys with m > 0: DSV_ERR_INVALID_ARGUMENT.  A dead set (its device shut
 *               down): DSV_ERR_NOT_INITIALIZED.  m = 0: DSV_OK, nothing launched.  k + m > capacity:
 *               DSV_ERR_TOO_LARGE, nothing launched, the set unchanged (so every m > 0 on a set of a plain
 *               constructor).  On any error the set keeps its k and every verdict under it.
 *   Calls in flight and captured graphs (the stale-k rule)   No device pointer of a set ever changes, and an
 *               append writes only table, key_ok and key-byte rows >= the old k and index slots that were empty.
 *               A keyed call carries the k it was enqueued with, a captured graph the k of its capture, for ever:
 *               an index >= that k gives ok = 0, and the lookup reads an index slot that holds a newer key as
 *               empty.  So such a call decides exactly as it would have before the append — the closed-set forms
 *               reject items under newer keys, the open-set form sends them down the unkeyed path and returns the
 *               same verdict.  To use the new keys from a graph, capture it again.
 *   Sizes       workspaces that depend on k (dsv_keyed_rlc_workspace_bytes) are checked against the k the call
 *               sees: size them for `capacity`.
 * Eviction is replacement: "keys replaced in place", next.  Not here: retiring a key without a successor, growing
 * past the capacity. */
int dsv_keyset_create_reserved(int scheme, const uint8_t *pk_uv, const uint8_t *pk2_uv, size_t k, size_t capacity,
                               dsv_keyset **out);
int dsv_keyset_append(dsv_keyset *ks, const uint8_t *pk_uv, const uint8_t *pk2_uv, size_t m, uint32_t *first_index);
int dsv_keyset_append_wire(dsv_keyset *ks, const uint8_t *pk_bytes, size_t m, uint32_t *first_index);
int dsv_keyset_capacity(const dsv_keyset *ks, size_t *capacity);
/* ---- keys replaced in place: the key cache's eviction ----------------------------------
 * A full set (k == capacity) takes a new busy key in the place of an idle one, at the cost of the new key's own
 * table, instead of a second set over all keys: no allocation moves; k, the capacity and every other key's index,
 * table and verdict stay as they are; captured graphs stay valid.
 *   replace     `indices`: a host array of m pairwise distinct indices, each < k; key j of the call takes the place
 *               of key indices[j].  The keys come in the constructor's form (replace: affine host bytes;
 *               replace_wire: key records, decoded by the device decoder exactly as dsv_keyset_append_wire does)
 *               and are validated and recorded as at creation: an invalid or undecodable key gets key_ok = 0, keeps
 *               the index and is in neither index over the keys' values.
 *   Checks      in this order, all before anything is launched or written: NULL handle, a handle that is not
 *               live (DSV_ERR_INVALID_ARGUMENT; the former also before dsv_init), a dead set
 *               (DSV_ERR_NOT_INITIALIZED), m == 0 (DSV_OK), NULL `indices` or keys, an index >= k or an index
 *               given twice (DSV_ERR_INVALID_ARGUMENT).  On each of them the set is unchanged.
 *   Contract    The call blocks.  When it has returned, every keyed call enqueued afterwards, on any stream of the
 *               set's device, sees the new keys at those indices: by index, ok[i] is the unkeyed verdict under the
 *               new key; by value, the old key is a miss unless an equal key is registered at another index, and the
 *               new key looks up to the lowest index of an equal valid key.  The open-set forms keep returning the
 *               unkeyed call's verdict for every input, before and after.  Replaces and appends to one set are
 *               serialised.
 *   Calls in flight   The call quiesces.  It first builds the new keys' tables in a scratch of its own, on a stream
 *               of its own, while verify calls go on.  Then it takes the library's key-set lock exclusively, so no
 *               library call is enqueueing on any key set, and waits for the set's device (hipDeviceSynchronize)
 *               before the first byte of the set changes; the lock is released when the set is complete again.  A
 *               call enqueued before the replace decides on the old set and a call enqueued after it on the new; no
 *               call sees a mixture.  Two duties are the caller's: no graph that holds the set may be replayed
 *               while the replace runs (graph launches do not pass through the library's lock), and no stream of
 *               the device may be capturing then (a device-wide wait is illegal during a capture).
 *   Captured graphs   A graph captured earlier stays valid afterwards.  It keeps its k: at a replaced index below
 *               that k it sees the new key, by index and by value; keys at indices >= its k stay misses.  Both
 *               indices over the keys' values are rebuilt in the layout that inserting key 0, then 1, and so on
 *               gives, so the stale-k rule above holds for every k, not only for the k of an append.
 *   Failures    A HIP failure before the set is written leaves it unchanged.  A HIP failure while it is written
 *               leaves the set dead — its device memory freed, every later call on it DSV_ERR_NOT_INITIALIZED,
 *               dsv_keyset_destroy releases the handle — and returns the error.
 *   Sizes       no device allocation changes: dsv_keyset_bytes, dsv_keyset_index_bytes and
 *               dsv_keyset_wire_index_bytes are what they were. */
int dsv_keyset_replace(dsv_keyset *ks, const uint32_t *indices, const uint8_t *pk_uv,
                       const uint8_t *pk2_uv, size_t m);
int dsv_keyset_replace_wire(dsv_keyset *ks, const uint32_t *indices, const uint8_t *pk_bytes, size_t m);
size_t dsv_keyed_workspace_bytes(size_t n);
int dsv_verify_single_keyed_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *key_idx,
                                const void *m, size_t n, void *ok, void *workspace, size_t workspace_bytes,
                                void *stream);
int dsv_verify_double_keyed_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *Rp_uv,
                                const void *key_idx, const void *m, size_t n, void *ok, void *workspace,
                                size_t workspace_bytes, void *stream);
int dsv_verify_vargen_keyed_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *key_idx,
                                const void *m, size_t n, void *ok, void *workspace, size_t workspace_bytes,
                                void *stream);
int dsv_verify_single_keyed(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv,
                            const uint32_t *key_idx, const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_keyed(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv, const uint8_t *Rp_uv,
                            const uint32_t *key_idx, const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_vargen_keyed(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv,
                            const uint32_t *key_idx, const uint8_t *m, size_t n, uint8_t *ok);
/* ---- keyed wire form: serialized signatures against a registered key set -----------
 * The signatures arrive as the reference's `Signature::to_bytes()` records — sig64 = u || R (single,
 * var-generator), sig96 = u || R || R' (double), nonce points compressed — and the key by its index in `ks`.
 * One decode launch (u copied out, the nonce points decompressed, one validity byte per item), then the
 * challenge hash and the keyed kernel: three launches, one stream.
 *   Verdicts    ok[i] = 1 iff `Signature*::from_bytes(sig_i)` would succeed, key_idx[i] is in range, the key
 *               is valid and `verify` returns true: ok[i] equals dsv_verify_*_keyed_dev's verdict on
 *               (u_i, decompress(R_i)[, decompress(R'_i)], key_idx[i], m_i) AND-ed with the decode flags of the
 *               item's nonce points (dsv_decompress_points_dev's: v < q, u^2 d == n, root by the sign bit, no
 *               further canonicity or subgroup test).  For a set whose keys are all valid this is also
 *               dsv_verify_*_wire's verdict on (sig_i, to_bytes(key[key_idx[i]]), m_i).
 *   Arguments   everything the keyed _dev calls promise: a short workspace, a scheme mismatch, a key set of
 *               another device (the owner of `ok`), a NULL pointer with n > 0: DSV_ERR_INVALID_ARGUMENT and
 *               nothing launched; a dead set: DSV_ERR_NOT_INITIALIZED; n = 0: DSV_OK; an index >= k gives 0
 *               and reads no table.  In addition `sig` must be 16-byte aligned (DSV_ERR_INVALID_ARGUMENT).
 *   Enqueue-only the _dev calls never synchronise and order on `stream`.
 *   Workspace   workspace_bytes >= dsv_keyed_wire_workspace_bytes(scheme, n) (device, 256-byte aligned) =
 *               the decoded columns u (32 B), R (64 B)[, R' (64 B)] and the decode flags (1 B per item), then
 *               dsv_keyed_workspace_bytes(n); each part rounded up to 256 B; never smaller for a larger n; no
 *               GPU needed; 0 for an unknown scheme.
 *   Host forms  take host arrays (pageable or pinned) and run on the key set's device through the chunked
 *               host pipeline of the other host entry points (copy and compute overlap; dsv_set_host_threads
 *               and the two-calls-in-flight rule apply); they block, and a set cannot be destroyed or shut
 *               down under a running call. */
size_t dsv_keyed_wire_workspace_bytes(int scheme, size_t n);
int dsv_verify_single_keyed_wire_dev(const dsv_keyset *ks, const void *sig64, const void *key_idx, const void *m,
                                     size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream);
int dsv_verify_double_keyed_wire_dev(const dsv_keyset *ks, const void *sig96, const void *key_idx, const void *m,
                                     size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream);
int dsv_verify_vargen_keyed_wire_dev(const dsv_keyset *ks, const void *sig64, const void *key_idx, const void *m,
                                     size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream);
int dsv_verify_single_keyed_wire(const dsv_keyset *ks, const uint8_t *sig64, const uint32_t *key_idx,
                                 const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_double_keyed_wire(const dsv_keyset *ks, const uint8_t *sig96, const uint32_t *key_idx,
                                 const uint8_t *m, size_t n, uint8_t *ok);
int dsv_verify_vargen_keyed_wire(const dsv_keyset *ks, const uint8_t *sig64, const uint32_t *key_idx,
                                 const uint8_t *m, size_t n, uint8_t *ok);
/* ---- keyed typed-object form: the reference's in-memory objects against a registered key set --
 * Keys are registered from `PublicKey*` objects where they lie, `Signature*` objects are verified where they lie
 * by key index: Montgomery limbs and projective points as described under "the reference's IN-MEMORY
 * representation" above (scalar 32 B; point 96 B = limbs of u || v || z of the JubJubExtended, t1 / t2 never
 * read).  The key set carries its scheme, so there is one entry point per form.  No kernel of its own: the
 * normalisation launch of the *_mont forms over the nonce points alone (it converts u and m as well), then the
 * challenge hash and the keyed kernel — three launches, one stream; in the constructor the same normalisation
 * over the key points in front of the table build.
 *   create_mont_cols  cols[0] = PK, cols[1] = PK' (double) / Gen (var-generator): key j's point at base + j *
 *               stride, stride >= 96 (sizeof of the key object).  A key is valid iff every limb group is < q,
 *               z != 0 and the normalised point is on the curve (dsv_keyset_key_ok).  The set is the one
 *               dsv_keyset_create builds from the normalised keys: same key_ok, same table entries.  Runs on
 *               the current device (it must be initialised) and blocks, like the other constructors.
 *   Columns     verify: single / var-generator u, R, key_idx, m [4]; double u, R, R', key_idx, m [5]; widths 32,
 *               96, (96), 4, 32; item i at base + i * stride, stride >= width; key_idx (uint32) 4-byte aligned,
 *               its stride a multiple of 4.  A violation: DSV_ERR_INVALID_ARGUMENT, "column k: ...".
 *   Verdicts    ok[i] equals dsv_verify_*_mont's verdict on (u_i, R_i[, R'_i], key[key_idx[i]], m_i) for every
 *               input the Rust types can hold, and dsv_verify_*_keyed_dev's on the `to_bytes()` /
 *               `to_hash_inputs()` of the same values.  Limbs not below their modulus, z = 0, an index >= k or
 *               an invalid key give 0; an index >= k reads no table.
 *   _dev form   everything the keyed _dev calls promise: a short workspace, a key set of another device (the
 *               owner of `ok`), a NULL pointer with n > 0: DSV_ERR_INVALID_ARGUMENT, nothing launched, `ok`
 *               untouched; a dead set: DSV_ERR_NOT_INITIALIZED; n = 0: DSV_OK.  Rp_uvz is required for a double
 *               set and ignored otherwise.  Enqueue-only, ordered on `stream`, may be captured.
 *   Workspace   workspace_bytes >= dsv_keyed_mont_workspace_bytes(scheme, n) (device, 256-byte aligned) = the
 *               normalised columns u (32 B), m (32 B), R (64 B)[, R' (64 B)], the validity bytes (1 B per item),
 *               the normalisation's prefix products (points * (n + 32) * 36 B), then
 *               dsv_keyed_workspace_bytes(n); each part rounded up to 256 B; never smaller for a larger n; no GPU
 *               needed; 0 for an unknown scheme.
 *   Host form   reads the objects where they lie and runs on the key set's device through the chunked host
 *               pipeline (one normalisation launch per chunk, hash + keyed kernel per sub-batch; copy and compute
 *               overlap; dsv_set_host_threads and the two-calls-in-flight rule apply); blocks; a set cannot be
 *               destroyed or shut down under a running call.
 *   Submit      as dsv_verify_*_mont_cols_submit: returns at once with a dsv_job for dsv_job_wait / dsv_job_done;
 *               cols[] is copied, the objects and `ok` must stay valid until the wait returns.  The job holds the
 *               set from before submit returns: dsv_keyset_destroy and dsv_shutdown* wait for it.  A job whose
 *               set died before it ran reports DSV_ERR_NOT_INITIALIZED at its wait. */
int dsv_keyset_create_mont_cols(int scheme, const dsv_column *cols /*[1|2]*/, size_t k, dsv_keyset **out);
/* dsv_keyset_append for key objects (cols as for create_mont_cols; "key sets that grow" above) */
int dsv_keyset_append_mont_cols(dsv_keyset *ks, const dsv_column *cols /*[1|2]*/, size_t m, uint32_t *first_index);
size_t dsv_keyed_mont_workspace_bytes(int scheme, size_t n);
int dsv_verify_keyed_mont_dev(const dsv_keyset *ks, const void *u, const void *R_uvz,
                              const void *Rp_uvz /* double only, else NULL */, const void *key_idx, const void *m,
                              size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream);
int dsv_verify_keyed_mont_cols(const dsv_keyset *ks, const dsv_column *cols /*[4|5]*/, size_t n, uint8_t *ok);
int dsv_verify_keyed_mont_cols_submit(const dsv_keyset *ks, const dsv_column *cols /*[4|5]*/, size_t n, uint8_t *ok,
                                      dsv_job **job);
/* ---- key sets by key VALUE: look the keys up on the device, closed-set verify ----------
 * Callers hold (signature, public key, message) triples, not indices.  Every key set carries an index over its
 * own keys — built by all three constructors behind the tables, in a device allocation of its own:
 * dsv_keyset_bytes and dsv_keyset_info's `bytes` do not count it, dsv_keyset_index_bytes(scheme, k) does (no GPU
 * needed; 0 for an unknown scheme or k = 0; a reserved set: of its capacity) = the keys' canonical affine bytes (64 B per point, key-major, rounded
 * up to 256) + an open-addressing table of `cap` uint32 slots (rounded up to 256), cap = the smallest power of two
 * >= max(64, 2k), linear probing from a home slot (dsv_debug_keyset_home_slot; an unsalted hash of the key's
 * 32-bit words) that wraps.  A match is always a comparison of all the key's bytes; the hash only picks where the
 * walk starts, and no walk is longer than the number of registered keys plus one.
 *   Keys        key_a = PK (64 B affine u || v per item), key_b = PK' (double) / Gen (var-generator); key_b is
 *               ignored and may be NULL for a single set.
 *   Lookup      key_idx_out[i] = the LOWEST index of a VALID registered key (dsv_keyset_key_ok: 1) whose bytes
 *               equal item i's key bytes, else DSV_KEY_NONE.  A key registered but invalid never matches, nor do
 *               other encodings of a registered key's residues (u + q), its negation, or a registered PK paired
 *               with another key's second point.  misses (may be NULL): _dev form one 4-byte-aligned uint32 on
 *               the set's device, zeroed on the stream and then SET to the number of DSV_KEY_NONE items; host
 *               form a size_t.
 *   Verify      ok[i] = [item i's key bytes are those of a valid registered key] & (the unkeyed entry point's
 *               verdict on (u, R[, R'], key, m)) = dsv_verify_*_keyed_dev's verdict at the looked-up index, and 0
 *               on a miss (DSV_KEY_NONE >= k reads no table).  A MISS IS A REJECTION, NOT AN ERROR: this is verify
 *               against a closed set — a signature under a key that is not in the set does not pass, however
 *               valid it is under its own key.  The set carries its scheme: one entry point per residency; Rp_uv
 *               is required for a double set and ignored otherwise.
 *   _dev forms  the checks of the keyed _dev calls in their order: a dead set DSV_ERR_NOT_INITIALIZED; n = 0
 *               DSV_OK with nothing enqueued; a NULL pointer with n > 0 (key_b of a two-point set included), a
 *               short workspace, outputs that are not on the set's device: DSV_ERR_INVALID_ARGUMENT, nothing
 *               launched, `ok` untouched.  Enqueue-only on `stream`, never synchronise, may be captured: the
 *               lookup, the challenge hash, the keyed kernel — three kernel launches, in front of them a one-lane
 *               kernel that zeroes `misses` when it is given; on an empty set (k = 0) two fills stand in for the lookup
 *               kernel (every index DSV_KEY_NONE, misses = n).
 *   Alignment   the lookup kernel reads a key in 16-byte loads: the device key columns must be 16-byte aligned
 *               (DSV_ERR_INVALID_ARGUMENT otherwise, nothing launched); key_idx_out and misses 4-byte aligned.
 *               The host forms stage the columns themselves and accept any alignment.
 *   Workspace   dsv_keyed_lookup_workspace_bytes(n) = the index column (4 B per item, rounded up to 256) +
 *               dsv_keyed_workspace_bytes(n); device, 256-byte aligned; no GPU needed.
 *   Host forms  take host arrays, stage in chunks on the key set's device and block.
 *   Before dsv_init there is no handle to give: a call of this group with a NULL handle then returns
 *   DSV_ERR_NOT_INITIALIZED (afterwards a NULL handle is DSV_ERR_INVALID_ARGUMENT, as for every keyed call). */
#define DSV_KEY_NONE 0xFFFFFFFFu
size_t dsv_keyset_index_bytes(int scheme, size_t k);
int dsv_keyset_lookup_dev(const dsv_keyset *ks, const void *key_a, const void *key_b, size_t n, void *key_idx_out,
                          void *misses, void *stream);
int dsv_keyset_lookup(const dsv_keyset *ks, const uint8_t *key_a, const uint8_t *key_b, size_t n,
                      uint32_t *key_idx_out, size_t *misses);
size_t dsv_keyed_lookup_workspace_bytes(size_t n);
int dsv_verify_keyed_lookup_dev(const dsv_keyset *ks, const void *u, const void *R_uv,
                                const void *Rp_uv /* double only, else NULL */, const void *key_a,
                                const void *key_b /* NULL for single */, const void *m, size_t n, void *ok,
                                void *workspace, size_t workspace_bytes, void *stream, void *misses);
int dsv_verify_keyed_lookup(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv, const uint8_t *Rp_uv,
                            const uint8_t *key_a, const uint8_t *key_b, const uint8_t *m, size_t n, uint8_t *ok,
                            size_t *misses);
/* introspection: the home slot of a key in the index of a set of k keys (no GPU needed; all ones for an unknown
 * scheme, k = 0 or a NULL key): with words = the 32-bit little-endian words of key_a, then those of key_b,
 *   h = 0;  for w in words: h = (h ^ w) * 0x9E3779B1;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;
 *   h *= 0xC2B2AE35;  h ^= h >> 16   (mod 2^32);  home = h & (cap - 1) */
uint64_t dsv_debug_keyset_home_slot(int scheme, size_t k, const uint8_t *key_a, const uint8_t *key_b);
/* introspection: out[0] = slots of the index, [1] = occupied slots (= distinct valid keys), [2] = occupied slots whose key
 * is not in its home slot, [3] = the longest probe of a registered key (slots read to find it; 1 = at home);
 * all 0 for an empty set */
int dsv_debug_keyset_index_stats(const dsv_keyset *ks, uint64_t out[4]);
/* introspection: copies the slot array of one index (form 0 = affine, 1 = record) to the host:
 * writes min(slots, room) uint32 and reports the slot count in *slots_out (may be NULL); a slot holds a key index
 * or DSV_KEY_NONE.  Blocks; a NULL handle is DSV_ERR_NOT_INITIALIZED before dsv_init and
 * DSV_ERR_INVALID_ARGUMENT after it, as is an unknown form. */
int dsv_debug_keyset_slots(const dsv_keyset *ks, int form, uint32_t *out, size_t room, size_t *slots_out);
/* introspection: host nanoseconds the latest dsv_keyset_replace* of this process held the key-set lock exclusively
 * (the device-wide wait, the commit, the index rebuild); 0 before the first */
uint64_t dsv_debug_keyset_replace_exclusive_ns(void);
/* ---- key sets as a key cache: open-set verify by key value -----------------------------
 * The caller that verifies (signature, public key, message) triples as they arrive, most under a few busy keys
 * and some under keys it has never seen.  Same arguments as dsv_verify_keyed_lookup[_dev]; what differs is what a
 * miss means:
 *   Verify      ok[i] = what dsv_verify_single_dev / dsv_verify_double_dev writes for the same columns, for every
 *               input.  An item whose key bytes are those of a valid registered key is decided by that key's
 *               tables; every other item (an unregistered key, a registered but invalid one, another encoding of
 *               a registered key) is decided by the unkeyed equation, in the same call.  Registering a key changes
 *               how fast a verdict arrives and never the verdict.  misses: as for the closed-set call — the number
 *               of items that took the unkeyed path.
 *   Schemes     single and double sets through dsv_verify_keyed_open[_dev]; a var-generator set there is
 *               DSV_ERR_INVALID_ARGUMENT (nothing launched): it has calls of its own, below.
 *   _dev form   checks, error codes and alignment rules of dsv_verify_keyed_lookup_dev.  Enqueue-only on `stream`,
 *               one straight chain, never synchronises, may be captured: the lookup, the challenge hash over all n
 *               (once, for both paths), the keyed kernel over all n (a miss reads no table and gets 0), a one-lane
 *               kernel that zeroes the list's length and the miss list (the positions of the DSV_KEY_NONE items, one atomic per wave), and
 *               the unkeyed equation over that list, which overwrites the 0 of exactly the listed items.  The last
 *               launch is sized for n items and reads the list's length on the device: a workgroup past the end
 *               returns at once, so the host never learns the number of misses.  An empty set (k = 0): every
 *               item takes the unkeyed path.
 *   Workspace   dsv_keyed_open_workspace_bytes(n) = dsv_keyed_lookup_workspace_bytes(n) + the miss list (4 B per
 *               item, rounded up to 256) + 256 (its length) + the unkeyed kernel's per-lane window tables
 *               (min(ceil(n / 64), 4096) * 64 lanes * 3888 B); device, 256-byte aligned; no GPU needed.
 *   Host form   host arrays, staged in chunks of 2^18 items on the key set's device; blocks; *misses is the sum
 *               over the chunks. */
size_t dsv_keyed_open_workspace_bytes(size_t n);
int dsv_verify_keyed_open_dev(const dsv_keyset *ks, const void *u, const void *R_uv,
                              const void *Rp_uv /* double only, else NULL */, const void *key_a,
                              const void *key_b /* NULL for single */, const void *m, size_t n, void *ok,
                              void *workspace, size_t workspace_bytes, void *stream, void *misses);
int dsv_verify_keyed_open(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv, const uint8_t *Rp_uv,
                          const uint8_t *key_a, const uint8_t *key_b, const uint8_t *m, size_t n, uint8_t *ok,
                          size_t *misses);
/* The var-generator scheme's open-set form: (SignatureVarGen, PublicKeyVarGen, message) triples, the key columns
 * PK_uv / Gen_uv being what the closed-set call takes as key_a / key_b.
 *   Verify      ok[i] = what dsv_verify_vargen_dev writes for the same (u, R, PK, Gen, m) columns, for every input.
 *               An item whose (PK, Gen) bytes are those of a valid registered key is decided by that key's tables;
 *               every other item — an unregistered pair, a registered PK beside another key's Gen, a registered
 *               but invalid key, another encoding — by the unkeyed equation u*Gen + c*PK == R, in the same call.
 *               misses: as for the closed-set call.
 *   Schemes     var-generator sets only; a single or double set is DSV_ERR_INVALID_ARGUMENT (nothing launched; the
 *               message names dsv_verify_keyed_open).
 *   _dev form   checks, error codes, texts and alignment rules of dsv_verify_keyed_open_dev, and its chain of
 *               launches on `stream` with the three-base one-lane kernel over the miss list at the end;
 *               enqueue-only, never synchronises, may be captured.  n = 0: DSV_OK, nothing touched.
 *   Workspace   dsv_keyed_open_workspace_bytes(n), the same layout (its window tables are the three per lane that
 *               this scheme's unkeyed kernel needs).
 *   Host form   as dsv_verify_keyed_open: chunks of 2^18 items, *misses summed over the chunks. */
int dsv_verify_vargen_keyed_open_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *PK_uv,
                                     const void *Gen_uv, const void *m, size_t n, void *ok, void *workspace,
                                     size_t workspace_bytes, void *stream, void *misses);
int dsv_verify_vargen_keyed_open(const dsv_keyset *ks, const uint8_t *u, const uint8_t *R_uv, const uint8_t *PK_uv,
                                 const uint8_t *Gen_uv, const uint8_t *m, size_t n, uint8_t *ok, size_t *misses);
/* ---- the key cache for serialized records: open-set verify by compressed key ----------
 * The caller of dsv_verify_keyed_open* usually holds its triples serialized: `Signature*::to_bytes()` records
 * (sig64 = u || R, sig96 = u || R || R', nonce points compressed) and `PublicKey*::to_bytes()` records (pk32 = pk;
 * pk64 = pk || pk' for the double scheme, pk || gen for the var-generator scheme; 32 B per point, compressed).
 * Every key set carries a second index, over the compressed records of its own valid keys, built by every
 * constructor and every append behind the affine index, in a device allocation of its own, made once for the
 * set's capacity: dsv_keyset_bytes, dsv_keyset_index_bytes and dsv_keyset_info's `bytes` do not count it,
 * dsv_keyset_wire_index_bytes(scheme, k) does (no GPU needed; 0 for an unknown scheme or k = 0; a reserved set: of
 * its capacity) = the records (32 B per point, key-major, rounded up to 256) + as many uint32 slots as the affine
 * index has (rounded up to 256), probed the same way from a home slot of its own
 * (dsv_debug_keyset_wire_home_slot).  The record of a valid key is v with bit 255 set to the lowest bit of u — a
 * pure function of its affine bytes — so a registered key is found by byte comparison and never decompressed;
 * only the keys of the items that miss pay for a square root.
 *   Lookup      key_idx_out[i] = the LOWEST index of a VALID registered key (dsv_keyset_key_ok: 1) whose canonical
 *               compressed record equals item i's key record byte for byte, else DSV_KEY_NONE: what
 *               dsv_keyset_lookup writes for the decompressed keys whenever the record is the canonical one.  Every
 *               other record is a miss, not an error: another encoding of a registered point (u = 0 with the sign
 *               bit set), v >= q, a non-square, a registered key's pk beside another key's gen, the record of a key
 *               that was registered but is invalid.  misses as for dsv_keyset_lookup[_dev].
 *   Verify      ok[i] = what dsv_verify_*_wire_dev writes for the same records, for every input: 1 iff every
 *               `from_bytes` would succeed and `verify()` would return true.  Registering a key changes how fast the
 *               verdict arrives and never the verdict.  misses: the number of items that took the unkeyed path.
 *   _dev forms  checks and error codes of the keyed _dev calls in their order (a dead set DSV_ERR_NOT_INITIALIZED;
 *               a set of another scheme DSV_ERR_INVALID_ARGUMENT; n = 0 DSV_OK with nothing enqueued; a NULL
 *               pointer with n > 0, a short workspace, outputs that are not on the set's device:
 *               DSV_ERR_INVALID_ARGUMENT), then alignment: `sig` and `pk` 16-byte aligned, key_idx_out and misses
 *               4-byte aligned (DSV_ERR_INVALID_ARGUMENT).  On any error nothing is launched and nothing written.
 *               Enqueue-only on `stream`, one straight chain, never synchronise, may be captured: the decode of the
 *               signatures (dsv_verify_*_keyed_wire_dev's), the lookup of the key records, the challenge hash and
 *               the keyed kernel over all n (a miss gets 0 there), the miss list, the decompression of the listed
 *               items' key records (dsv_decompress_points_dev's arithmetic and bytes; its flag is AND-ed into the
 *               item's validity), and the unkeyed equation over the list.  The last two launches are sized for n
 *               items and read the list's length on the device.  A call carries the k it was enqueued with (the
 *               stale-k rule of "key sets that grow"); an empty set (k = 0): every item takes the unkeyed path.
 *   Workspace   dsv_keyed_open_wire_workspace_bytes(scheme, n) = (dsv_keyed_wire_workspace_bytes(scheme, n) -
 *               dsv_keyed_workspace_bytes(n)) [the decoded signature columns] + the key columns of the misses (64 B
 *               per item and key point, each column rounded up to 256) + dsv_keyed_open_workspace_bytes(n); device,
 *               256-byte aligned; no GPU needed; 0 for an unknown scheme.
 *   Host forms  host arrays, staged in chunks of 2^18 items on the key set's device (any alignment); block;
 *               *misses is the sum over the chunks.
 *   Before dsv_init a call of this group with a NULL handle returns DSV_ERR_NOT_INITIALIZED. */
size_t dsv_keyset_wire_index_bytes(int scheme, size_t k);
int dsv_keyset_lookup_wire_dev(const dsv_keyset *ks, const void *pk_records, size_t n, void *key_idx_out,
                               void *misses, void *stream);
int dsv_keyset_lookup_wire(const dsv_keyset *ks, const uint8_t *pk_records, size_t n, uint32_t *key_idx_out,
                           size_t *misses);
/* introspection: *slot = the home slot of a key record (32 B per key point) in the wire index of a set of
 * `capacity` keys (no GPU needed): dsv_debug_keyset_home_slot's hash over the record's 8 (16) little-endian 32-bit
 * words, & (cap - 1).  Unknown scheme, capacity = 0 or a NULL pointer: DSV_ERR_INVALID_ARGUMENT. */
int dsv_debug_keyset_wire_home_slot(int scheme, size_t capacity, const uint8_t *record, uint64_t *slot);
size_t dsv_keyed_open_wire_workspace_bytes(int scheme, size_t n);
int dsv_verify_single_keyed_open_wire_dev(const dsv_keyset *ks, const void *sig64, const void *pk32, const void *m,
                                          size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream,
                                          void *misses);
int dsv_verify_double_keyed_open_wire_dev(const dsv_keyset *ks, const void *sig96, const void *pk64, const void *m,
                                          size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream,
                                          void *misses);
int dsv_verify_vargen_keyed_open_wire_dev(const dsv_keyset *ks, const void *sig64, const void *pk64, const void *m,
                                          size_t n, void *ok, void *workspace, size_t workspace_bytes, void *stream,
                                          void *misses);
int dsv_verify_single_keyed_open_wire(const dsv_keyset *ks, const uint8_t *sig64, const uint8_t *pk32,
                                      const uint8_t *m, size_t n, uint8_t *ok, size_t *misses);
int dsv_verify_double_keyed_open_wire(const dsv_keyset *ks, const uint8_t *sig96, const uint8_t *pk64,
                                      const uint8_t *m, size_t n, uint8_t *ok, size_t *misses);
int dsv_verify_vargen_keyed_open_wire(const dsv_keyset *ks, const uint8_t *sig64, const uint8_t *pk64,
                                      const uint8_t *m, size_t n, uint8_t *ok, size_t *misses);
/* ---- the key cache for typed objects: open-set verify of verify_batch's arguments --------
 * The caller that holds the reference's in-memory types and calls verify_batch(&[Signature], &[PublicKey],
 * &[BlsScalar]): Montgomery limbs and projective points as described under "the reference's IN-MEMORY
 * representation" above (scalar 32 B; point 96 B = limbs of u || v || z, t1 / t2 never read).  The key set carries
 * its scheme, so there is one entry point per form.
 *   Columns     those of dsv_verify_*_mont_cols, in their order and widths: single u, R, PK, m [4]; double u, R, R',
 *               PK, PK', m [6]; var-generator u, R, PK, Gen, m [5]; widths 32 / 96 / 32.  The _dev form takes them as
 *               arguments: key_a_uvz = PK, key_b_uvz = PK' (double) / Gen (var-generator), NULL and ignored for a
 *               single set; Rp_uvz is required for a double set and ignored otherwise.
 *   Verdicts    ok[i] = what dsv_verify_{single,double,vargen}_mont_dev writes for the same limbs, for every input.
 *               Limbs not below their modulus and z = 0 give 0.  Registering a key changes how fast a verdict
 *               arrives and never the verdict.
 *   Hit         the item's key limbs are usable (every limb group < q, every z != 0) and its normalised affine bytes
 *               (u/z, v/z, canonical) equal, byte for byte, those of a VALID registered key — the pair (PK, PK') for
 *               the double scheme, (PK, Gen) for the var-generator scheme; the lowest such index wins.  The item's z
 *               and the route by which the key was registered (affine, wire, typed, appended, replaced) do not
 *               matter.  A hit is decided by that key's tables.  Every other item is a miss, not an error — an
 *               unregistered key, a registered but invalid key, a registered PK beside another key's PK' / Gen, a
 *               point off the curve, unusable key limbs — and is decided by the unkeyed equation in the same call.
 *   misses      the number of items that took the unkeyed path, items with unusable key limbs INCLUDED (their
 *               verdict is 0 either way).  _dev form: may be NULL; else one 4-byte-aligned uint32 on the set's
 *               device, zeroed on the stream by a one-lane kernel and then added to.  Host form: a size_t, summed
 *               over the chunks and read back once at the end of the call; may be NULL.
 *   _dev form   checks, order, error codes and texts of dsv_verify_keyed_open_dev: a dead set
 *               DSV_ERR_NOT_INITIALIZED; n = 0 DSV_OK with nothing enqueued; a NULL pointer with n > 0 (key_b_uvz of
 *               a two-point set included), a short workspace, outputs that are not on the set's device:
 *               DSV_ERR_INVALID_ARGUMENT, nothing launched, `ok` untouched.  Alignment: the kernel loads limbs in
 *               16-byte loads — every input column must be 16-byte aligned, misses 4-byte aligned
 *               (DSV_ERR_INVALID_ARGUMENT otherwise, nothing launched).  Enqueue-only on `stream`, one straight
 *               chain, never synchronises, may be captured: ONE front kernel (normalisation of every point, the two
 *               scalar conversions, the lookup of the normalised key in the set's affine index), the challenge hash
 *               and the keyed kernel over all n (a miss gets 0 there), the miss list, the unkeyed equation over the
 *               list on the normalised key columns, of which only the rows of misses are ever written.  A call
 *               carries the k it was enqueued with (the stale-k rule of "key sets that grow"); an empty set (k = 0):
 *               every item takes the unkeyed path.  DSV_OPEN_MONT_FUSED=0 (read by dsv_init) runs the front as two
 *               launches — the *_mont forms' normalisation over all points, then dsv_keyset_lookup_dev's kernel —
 *               and a gate that makes an item with unusable key limbs a miss whatever its normalised bytes are:
 *               the same outputs for every input (A/B and cross-check).
 *   Workspace   dsv_keyed_open_mont_workspace_bytes(scheme, n) = the index column (4 B per item) + the miss list (4 B
 *               per item) + 256 (its length) + the unkeyed kernel's per-lane window tables (min(ceil(n / 64), 4096) *
 *               64 lanes * 3888 B) + the key columns of the misses (64 B per item and key point) + the normalised
 *               u (32 B), m (32 B), R (64 B)[, R' (64 B)] + the validity bytes (1 B per item) + the prefix products
 *               of all points (points * (n + 32) * 36 B, points = 2 / 4 / 3) + dsv_keyed_workspace_bytes(n); each
 *               part rounded up to 256 B, in this order: the index column is first, as in every by-value call;
 *               device, 256-byte aligned; never smaller for a larger n; no GPU needed; 0 for an unknown scheme.
 *   Host form   reads the objects where they lie and runs on the key set's device through the chunked host pipeline
 *               (one front launch per chunk; hash, keyed kernel and miss branch per sub-batch; copy and compute
 *               overlap; dsv_set_host_threads and the two-calls-in-flight rule apply); blocks; a set cannot be
 *               destroyed or shut down under a running call.  Column checks as dsv_verify_*_mont_cols ("column k:
 *               ...").
 *   Submit      as dsv_verify_keyed_mont_cols_submit: the job holds the set from before submit returns.  The
 *               submitted form reports no miss count.
 *   Before dsv_init a call of this group with a NULL handle returns DSV_ERR_NOT_INITIALIZED. */
size_t dsv_keyed_open_mont_workspace_bytes(int scheme, size_t n);
int dsv_verify_keyed_open_mont_dev(const dsv_keyset *ks, const void *u, const void *R_uvz,
                                   const void *Rp_uvz /* double only, else NULL */, const void *key_a_uvz,
                                   const void *key_b_uvz /* PK' | Gen, NULL for single */, const void *m, size_t n,
                                   void *ok, void *workspace, size_t workspace_bytes, void *stream, void *misses);
int dsv_verify_keyed_open_mont_cols(const dsv_keyset *ks, const dsv_column *cols /*[4|6|5]*/, size_t n, uint8_t *ok,
                                    size_t *misses /* may be NULL */);
int dsv_verify_keyed_open_mont_cols_submit(const dsv_keyset *ks, const dsv_column *cols /*[4|6|5]*/, size_t n,
                                           uint8_t *ok, dsv_job **job);
/* ---- key cache census: per-key hit counts and the distinct missed keys ---------------
 * What a cache needs in order to USE dsv_keyset_append* (admission) and dsv_keyset_replace* (eviction): which
 * registered keys are cold, which unregistered keys are busy.  The census answers both for one batch, on the
 * device, next to the verify call: the caller runs it over the key columns it hands to the open-set call, on the
 * same stream.  It changes no verdict and no other call; the lookup it repeats is that of dsv_keyset_lookup*.
 *   Keys        as for dsv_keyset_lookup_dev (key_a / key_b, 64 B affine per item), dsv_keyset_lookup_wire_dev
 *               (records, 32 B per key point) and dsv_verify_keyed_open_mont_dev (key_a_uvz / key_b_uvz, 96 B of
 *               Montgomery limbs u || v || z per item).
 *   key_idx_out may be NULL; else u32[n], exactly what dsv_keyset_lookup* of the same form writes (typed form: what
 *               the open typed call looks up — DSV_KEY_NONE for unusable key limbs).
 *   hits        may be NULL; else u32[capacity of the set] — sized for the capacity, so that a captured graph
 *               survives appends.  hits[j] is ADDED the number of items whose lookup result is j (the lowest index
 *               of an equal valid key).  A call touches only entries below the k it was enqueued with and never
 *               zeroes any: the caller owns the window (reset, decay).  The counts are uint32 and wrap.
 *   Miss        every item that is not a hit — an unregistered key, but also a key that is registered but invalid,
 *               another encoding of a registered key, a registered PK beside another key's second point.  All of
 *               them appear in the report, so A POLICY MUST EXPECT TO BE OFFERED SUCH KEYS: registering one again
 *               gives key_ok = 0 or changes nothing about the next lookup.
 *   Report      entries [0, totals[0]) of miss_rep / miss_count (u32[n] each; entries from totals[0] on are not
 *               written): one per DISTINCT missed key — compared by all its bytes — with miss_rep = the lowest
 *               item index that carries it (its bytes are at that row of the caller's own key columns) and
 *               miss_count = the number of items under it.  The _dev forms leave the order unspecified; the host
 *               forms return it sorted by count descending, then by representative ascending.
 *   totals      u32[4] (host forms: size_t[4]): [0] distinct missed keys, [1] missed items, [2] items with unusable
 *               key limbs (typed form: a limb group >= q or z = 0; they count in [1], have no key bytes to report
 *               and enter no report entry; the affine and record forms write 0), [3] reserved, written 0.  The sum
 *               of miss_count is totals[1] - totals[2].
 *   _dev forms  the checks of dsv_keyset_lookup_dev in their order and with their codes: a NULL handle before
 *               dsv_init DSV_ERR_NOT_INITIALIZED; n > DSV_MAX_BATCH DSV_ERR_TOO_LARGE; a dead set
 *               DSV_ERR_NOT_INITIALIZED; n = 0 DSV_OK with nothing enqueued; then, each DSV_ERR_INVALID_ARGUMENT
 *               with nothing launched and nothing written: a NULL pointer (key_b of a two-point set included;
 *               key_idx_out and hits may be NULL), key columns that are not 16-byte aligned, uint32 outputs that
 *               are not 4-byte aligned, a workspace that is not 16-byte aligned or shorter than
 *               dsv_keyset_census_workspace_bytes(n) (typed form: dsv_keyset_census_mont_workspace_bytes(scheme,
 *               n)), totals not on the set's device.  Enqueue-only on `stream`, never synchronise, may be captured:
 *               one straight chain of kernels — four one-lane stores that zero totals, the clearing of the call's
 *               miss table, (typed form: the *_mont forms' normalisation over the key points alone,) the census,
 *               the report; no memset node.  A call carries the k it was enqueued with (the stale-k rule of "key
 *               sets that grow"); on an empty set (k = 0) every item is a miss and nothing is walked.  The result
 *               is deterministic up to the order of the report.
 *   Workspace   dsv_keyset_census_workspace_bytes(n) = the miss table: `cap` uint32 slots and `cap` uint32 counts,
 *               cap = the smallest power of two >= max(64, 2n) (the slot count of a set of n keys, and the same home
 *               slot: dsv_debug_keyset_home_slot(scheme, n, ...) / dsv_debug_keyset_wire_home_slot(scheme, n, ...)
 *               predict where a missed key's walk starts), each rounded up to 256.  The typed form adds the
 *               normalised key columns (64 B per item and key point), the validity bytes (1 B per item) and the
 *               prefix products (points * (n + 32) * 36 B), each rounded up to 256; 0 for an unknown scheme.
 *               Device memory; never smaller for a larger n; no GPU needed.
 *   Host forms  take host arrays (typed form: cols[0] = PK, cols[1] = PK' / Gen objects, 96 B each, stride >= 96),
 *               stage in chunks of 2^18 items on the set's device, run the census per chunk and merge the chunk
 *               reports on the host by key bytes (typed form: by the normalised bytes), so the result is the whole
 *               call's: a representative is the lowest item index of the CALL.  hits is added to as by the _dev
 *               forms.  They block.
 *   DSV_CENSUS_LDS_KEYS=n (read by dsv_init): sets with at most n keys (default 4096, at most 16384) count their
 *               hits per workgroup in LDS, larger ones combine equal indices per wave; 0 sends every set down the
 *               per-wave path.  Same outputs either way (A/B and cross-check, like DSV_QUAD).
 *               dsv_debug_census_lds_keys(): the threshold as this process runs it. */
size_t dsv_keyset_census_workspace_bytes(size_t n);
size_t dsv_keyset_census_mont_workspace_bytes(int scheme, size_t n);
int dsv_keyset_census_dev(const dsv_keyset *ks, const void *key_a, const void *key_b /* NULL for single */, size_t n,
                          void *key_idx_out /* u32[n], may be NULL */,
                          void *hits /* u32[capacity], ADDED to, may be NULL */, void *miss_rep /* u32[n] */,
                          void *miss_count /* u32[n] */, void *totals /* u32[4] */, void *workspace,
                          size_t workspace_bytes, void *stream);
int dsv_keyset_census_wire_dev(const dsv_keyset *ks, const void *pk_records, size_t n, void *key_idx_out, void *hits,
                               void *miss_rep, void *miss_count, void *totals, void *workspace,
                               size_t workspace_bytes, void *stream);
int dsv_keyset_census_mont_dev(const dsv_keyset *ks, const void *key_a_uvz,
                               const void *key_b_uvz /* PK' | Gen, NULL for single */, size_t n, void *key_idx_out,
                               void *hits, void *miss_rep, void *miss_count, void *totals, void *workspace,
                               size_t workspace_bytes, void *stream);
int dsv_keyset_census(const dsv_keyset *ks, const uint8_t *key_a, const uint8_t *key_b, size_t n,
                      uint32_t *key_idx_out, uint32_t *hits, uint32_t *miss_rep, uint32_t *miss_count,
                      size_t totals[4]);
int dsv_keyset_census_wire(const dsv_keyset *ks, const uint8_t *pk_records, size_t n, uint32_t *key_idx_out,
                           uint32_t *hits, uint32_t *miss_rep, uint32_t *miss_count, size_t totals[4]);
int dsv_keyset_census_mont_cols(const dsv_keyset *ks, const dsv_column *cols /*[1|2]*/, size_t n,
                                uint32_t *key_idx_out, uint32_t *hits, uint32_t *miss_rep, uint32_t *miss_count,
                                size_t totals[4]);
int dsv_debug_census_lds_keys(void);
/* ---- keyed fast accept: the batch aggregate over a registered key set ----------------
 * Same inputs and the same verdict vector as dsv_verify_*_keyed_dev — ok[] equals theirs bit for bit; what
 * differs is the time.  Per group of up to 2^22 items (cut into sub-groups like the unkeyed fast accept), with
 * secret 128-bit weights z_i (z'_i) drawn per call (getrandom, ChaCha12), a sub-group is ACCEPTED iff
 *   (1) every R_i (R'_i) that enters the sum lies in the prime-order subgroup (r * S_p == O for the per-bit
 *       subset sums of the nonce points),
 *   (2) every key point an item of the sub-group references is torsion-free: r * PK_k == O (and r * PK'_k /
 *       r * Gen_k), from the key's own table, per call and only for referenced keys, and
 *   (3) single:  (sum z_i u_i) G + sum_k s_k PK_k - sum z_i R_i == O,   s_k = sum over key k of z_i c_i mod r
 *       double:  the same with (z'_i, G', s'_k, PK'_k, R'_i) added (two weights per item)
 *       vargen:  sum_k a_k Gen_k + sum_k s_k PK_k - sum z_i R_i == O,   a_k = sum over key k of z_i u_i mod r.
 * Accepted: every eligible item's verdict is `true` (error <= 2^-112 for a batch that holds a wrong
 * signature).  Malformed items — u >= r, a coordinate >= q, m >= q, idx >= k, key_ok[idx] == 0 — stay out
 * of the sum with verdict 0 (an index >= k never reads a table).  Anything else — a wrong signature, a torsion
 * component, an eligible R off the curve, a bin overflow — sends the sub-group to the keyed per-signature
 * kernel, which is enqueued behind the aggregate and returns at once where it accepted.
 * window_bits: 0 = automatic (groups below 2^19 items go straight to the keyed per-signature kernel: the
 * aggregate's tail does not pay below that), else one of 4, 6, 8, 12, 14, 16.
 * accepted: as for dsv_verify_single_rlc_dev (device-writable memory: written by a kernel; ordinary host
 * memory: the call waits for `stream` at its end).
 * workspace: workspace_bytes >= dsv_keyed_rlc_workspace_bytes(n, k, window_bits) (k: keys of the set;
 * 0 for bad bits; never less for a larger n or k).  Arguments as for the keyed _dev calls (short workspace,
 * scheme mismatch, wrong device, NULL with n > 0: DSV_ERR_INVALID_ARGUMENT, nothing launched; dead set:
 * DSV_ERR_NOT_INITIALIZED; n = 0: DSV_OK).
 * History: keyed calls keep counters of their own (dsv_debug_keyed_rlc_history) and never change
 * dsv_debug_rlc_history / _long; dsv_debug_rlc_subgroups applies to them too.
 * No graph capture: the weight key is drawn on the host per call, so a call on a capturing stream returns
 * DSV_ERR_INVALID_ARGUMENT with nothing enqueued (its first HIP call is hipStreamIsCapturing). */
size_t dsv_keyed_rlc_workspace_bytes(size_t n, size_t k, int window_bits);
/* the keyed plan of one group (no GPU needed): out[24] as dsv_rlc_plan_info's (no key windows: wpk = 0, no
 * long points), out[23] = workspace bytes of this plan for k keys */
int dsv_keyed_rlc_plan_info(int scheme, size_t n, size_t k, int window_bits, int groups, uint64_t *out /*[24]*/);
/* the device's keyed history counter (> 0: the next keyed calls run in sub-groups); set >= 0 overrides it */
int dsv_debug_keyed_rlc_history(int device, int set);
int dsv_verify_single_keyed_rlc_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *key_idx,
                                    const void *m, size_t n, void *ok, void *workspace, size_t workspace_bytes,
                                    void *stream, int window_bits, int *accepted);
int dsv_verify_double_keyed_rlc_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *Rp_uv,
                                    const void *key_idx, const void *m, size_t n, void *ok, void *workspace,
                                    size_t workspace_bytes, void *stream, int window_bits, int *accepted);
int dsv_verify_vargen_keyed_rlc_dev(const dsv_keyset *ks, const void *u, const void *R_uv, const void *key_idx,
                                    const void *m, size_t n, void *ok, void *workspace, size_t workspace_bytes,
                                    void *stream, int window_bits, int *accepted);
/* introspection: affine u || v (canonical LE) of digit * 2^(8*window) * point, point 0 = PK, 1 = PK' / Gen,
 * window 0 .. 31, digit -128 .. 128 */
int dsv_debug_keyset_entry(const dsv_keyset *ks, size_t key, int point, int window, int digit,
                           uint8_t out64[64]);

/* ---- introspection for tests: copy one fixed-base table entry (affine niels v+u, v-u, 2duv
 * as canonical LE, 96 B) for generator `which` (0 = G, 1 = G'), window w (signed windows of
 * dsv_fixed_window_bits() bits), digit magnitude d ---- */
int dsv_debug_table_entry(int which, int window, int digit, uint8_t out96[96]);
int dsv_fixed_window_bits(void); /* width of the (signed) fixed-base windows; digit <= 2^(bits-1) */
/* ---- introspection: the three short scalars of the var-generator kernel (lattice3.h) for (u, c):
 * per item 128 B = |x| || |y| || |z| (32 B LE each) || sign bytes of x, y, z || padding;
 * x = z*u, y = z*c (mod 8r), z odd.  u is taken mod 2^252, c mod 2^250. */
int dsv_debug_lattice3(const uint8_t *u, const uint8_t *c, size_t n, uint8_t *out128);
/* ---- introspection: the half-size scalars of the fixed-generator kernels (halfgcd.h) for c (taken
 * mod 2^250): per item 96 B = |a| || |b| (32 B LE each) || sign byte of b || padding;
 * a = b*c (mod 8r), b odd. */
int dsv_debug_half_scalars(const uint8_t *c, size_t n, uint8_t *out96);
/* ---- introspection: field-multiplier self test on the device: out = a*b mod q (canonical) */
int dsv_debug_fq_mul(const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* DSV_H */
