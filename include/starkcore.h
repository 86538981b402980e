/*
 * starkcore.h -- C ABI of the MI355X-native STARK polynomial core (libstarkcore.so).
 *
 * The reference (aszepieniec/stark-anatomy, pure Python) has no FFI; its boundary for this path is
 * the set of module-level callables in code/ntt.py, the fold expression in code/fri.py:85 and
 * code/merkle.py.  Each entry point below names the reference callable it replaces (file:line);
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - element = 16 bytes, two little-endian uint64 limbs (lo, hi), CANONICAL residue in [0, p),
 *     p = 1 + 407 * 2^119 (code/algebra.py:96-98); arrays contiguous, natural index order.
 *   - every function returns 0 on success or a negative SC_ERR_* code; sc_last_error() gives text.
 *     Nothing throws across the ABI; host-buffer calls block until the output buffer is valid.
 *   - host-buffer entry points (sc_ntt, ...) take caller-owned host memory.
 *   - *_dev entry points take device pointers (hipMalloc / torch tensor storage, 16-byte aligned) and
 *     a hipStream_t (NULL = the library's own stream) and are asynchronous on that stream.
 *   - sc_vec_t / sc_merkle_t are library-owned device objects behind opaque handles.
 *   - one context per PROCESS: sc_init(device) binds the process to one GPU (one process per GPU is the multi-GPU model,
 *     stark-anatomy_amd/sharded.py + torch.distributed/RCCL; there is no sc_init(ndev) -- a rank's share of the sharded
 *     transform is the sc_fourstep_* plan object below, driven by sharded.ShardedNtt).
 *   - streams: the library keeps a few scratch buffers (transform work space, temporaries) that every call reuses.  Calls
 *     that pass the SAME stream (or NULL) are ordered by that stream and need nothing else.  Calls on DIFFERENT streams must
 *     not overlap in time: order them with events, or synchronize, before switching streams (sharded.py does).  Frees of
 *     library objects never wait: the memory is parked behind an event on every stream in use (the library's and the caller
 *     streams seen so far) and goes back to the library's pool when those have completed.
 */
#ifndef STARKCORE_H
#define STARKCORE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_OK 0
#define SC_ERR_HIP (-1)              /* HIP runtime error (no GPU, OOM, launch failure) */
#define SC_ERR_NOT_POW2 (-2)         /* ntt.py:4 / merkle.py:7 "length must be power of two" */
#define SC_ERR_ROOT_ORDER (-3)       /* ntt.py:10 root^n != 1 */
#define SC_ERR_ROOT_NOT_PRIMITIVE (-4) /* ntt.py:11 root^(n/2) == 1 */
#define SC_ERR_DIV_ZERO (-5)         /* algebra.py:92 "divide by zero" */
#define SC_ERR_BAD_ARG (-6)
#define SC_ERR_UNSUPPORTED (-7)
#define SC_ERR_NOT_INIT (-8)
#define SC_ERR_TIMEOUT (-9)          /* a peer never arrived at a flag barrier of the direct-store corner turn: sticky until the plan's peers are set again */

typedef struct sc_vec sc_vec_t;        /* device-resident vector of field elements */
typedef struct sc_merkle sc_merkle_t;  /* device-resident BLAKE2b Merkle tree (all levels kept) */
typedef struct sc_merkle_forest sc_merkle_forest_t; /* device-resident forest of equal-sized Merkle trees over one matrix (all levels kept) */
typedef struct sc_later sc_later_t;    /* a check whose words arrive behind the work that produces them (sc_*_later_dev, sc_later_wait) */
typedef struct sc_polytree sc_polytree_t; /* device-resident subproduct tree over a list of points (all levels kept) */
typedef struct sc_geodomain sc_geodomain_t; /* tables of a domain that is a geometric progression first * ratio^i */

/* ---- lifecycle ---------------------------------------------------------------------------- */
int sc_device_count(void);
int sc_init(int device);               /* idempotent; selects the device and creates the library stream */
int sc_shutdown(void);                 /* frees plans, scratch and the stream */
const char* sc_last_error(void);
int sc_synchronize(void);              /* wait for the library stream */
/* The library stream as a raw hipStream_t, for callers that put their other device work on the same stream (no ordering needed
 * then), and a two-way, event-based ordering of the library stream with another stream that never blocks the host. */
int sc_stream(void** stream_out);
int sc_stream_join(void* other_stream);
/* tuning knobs for experiments (defaults are the measured optimum; -1 = choose by size where applicable): key in
 * {"max_tile_log","loge","max_col_log","min_tiles_log","single_pass_max_log","max_digit_log","direct_tw_max_log",
 *  "xcd_remap","fixed_shapes","merkle_big_nlev","wave_local","prio_balance","loge_cols","tw_on_load","prune","fast_fixups","fri_tail","fri_tail_stall","small_divisor_direct","verify_stage_kb","forest_four_lane_wgs","div_cols_chunk","div_cols_launch_log","tree_cols_launch_log","eval_chunk_log","eval_points_across_min","eval_across_min_products_log","rescue_tree_split_max_nodes","grind_window","grind_unrolled"}.  Plans are re-derived on the next
 * call; results never depend on the tuning ("fri_tail_stall" = k >= 0 is a test hook: the host withholds the challenge after round k of
 * the persistent tail kernel, whose wait then gives up after 2^13 polls; -1 = off; "small_divisor_direct" = 0: sc_coset_divide* transforms a
 * divisor of <= 8 coefficients like any other instead of evaluating it point by point; "verify_stage_kb" = the size of the staging buffer
 * of sc_merkle_verify_batch / sc_fri_colinearity_batch, 65536 by default, at least 16; "forest_four_lane_wgs" = a launch of a Merkle forest of
 * at most this many workgroups runs its narrow levels four lanes per BLAKE2b compression, 0 = never; "fast_fixups" = 1: the eight-element
 * batch kernel corrects by +-p on two limbs and repairs a dropped carry where it occurs, 0: exact arithmetic on every tile, 2: both
 * kernels on every tile (a test hook) -- see sc_ntt_columns_dev; "div_cols_chunk" = columns that share one batch inversion in
 * sc_pointwise_div_columns_later_dev / sc_coset_divide_columns_later_dev with a shared divisor, 0 = chosen by shape; "div_cols_launch_log" = log2 of the values
 * one set of launches of sc_coset_divide_columns_later_dev (and of sc_poly_divmod_columns_dev, sc_poly_mul_columns_dev, sc_poly_product_dev) takes, 26 by default and at most, at least 1: a test hook that makes the entry
 * work through a small matrix in several chunks of columns; "tree_cols_launch_log" = log2 of the elements one temporary of a set of columns of
 * sc_polytree_evaluate_columns_dev / sc_polytree_interpolate_columns_dev holds, 26 by default and at most, at least 1: a test hook that
 * makes those entries work through their columns in several sets; "eval_chunk_log" = log2 of the coefficients one workgroup of
 * sc_poly_eval_points_dev takes at least, 8 by default, 8 .. 24: a test hook that decides through how many chunks, and the launch that combines
 * them, a small input goes; "eval_points_across_min" = the number of points from which sc_poly_eval_points_dev takes its points-across-lanes kernel
 * instead of the coefficients-across-lanes one, 32 by default, at least 1; "eval_across_min_products_log" = log2 of the modular products
 * (m * k * cols) a call must have for that to apply, 26 by default, 0 .. 64 -- smaller calls do not fill the device and always spread a chunk
 * over a workgroup; 0 with "eval_points_across_min" = 1 takes the points-across-lanes kernel everywhere, which is how the tests reach it; "rescue_tree_split_max_nodes" = a level of a Rescue-Prime Merkle tree, or a batch of paths of sc_rescue_merkle_verify_batch or sc_rescue_merkle_path_trace_dev, of at most
 * this many nodes runs one lane per state register instead of one lane per node, 0 = never, 2147483647 = always, -1 = the default, 65536: the largest level width of the measured sweep at which that form is the faster one by more than the spread of the repetitions at every state width measured, profiles/rescue_merkle; the path trace has no key of its own: at depth 20 that form is the faster one at every batch measured up to 65536, profiles/rescue_membership; "grind_window" = the trials one launch of sc_grind / sc_grind_batch
 * tests per seed, -1 (or anything below 1) = the default, 4194304, from the sweep in profiles/grinding; results do not depend on it; "grind_unrolled" = 1: the
 * grinding kernel with rounds 1 .. 22 of the permutation fully unrolled instead of one loop over them, 0 = the default, an A/B knob).  Two keys manage the device-memory pool instead (freed vectors and trees are kept
 * on exact-size free lists, by default up to a quarter of the device's memory divided by the processes sharing the device;
 * environment STARKCORE_POOL_CAP_MB): "pool_cap_mb" = what the lists may keep from now on, "pool_trim" = hand everything on them
 * back to the device now (a caller whose own allocator -- torch's -- ran out of memory). */
int sc_set_tuning(const char* key, int value);
/* kernel launches (passes over the vector) one sc_ntt_dev of length n takes at the current tuning: 1 up to 2^11, 2 up to 2^20,
 * 3 up to 2^24, 4 beyond (0: n is not a power of two >= 2).  bench.py derives the algorithmic bytes per launch from it. */
int sc_ntt_num_passes(uint64_t n);
/* diagnostics (tools/pass_trace.py): while d_buf != NULL every geometry-specialised NTT pass launch writes 16 u64 per wave
 * (s_memtime at the phase boundaries of its workgroup; slot 15 = s_memrealtime at entry) to d_buf[(block*waves + wave)*16 ..];
 * the caller sizes the buffer for the launch it traces and passes NULL afterwards. */
int sc_debug_trace(void* d_buf);

/* diagnostics: out[i] = op(a[i], b[i]) computed by the device field routines the kernels use.
 * op 0: a*b*2^-128 (Montgomery product, b < p), 1: a+b, 2: a-b, 3: a*b, 4: a/2, 5: a^-1, 6: portable Montgomery product,
 * 7: the same product through the two-at-a-time routine of the butterflies with a, b in BOTH of its slots (all ones if its two
 * halves disagree; distinct operands per slot: sc_field_selftest2) */
int sc_field_selftest(int op, const void* a, const void* b, void* out, uint64_t n);
/* diagnostics: the two-slot and the top-limb-correction ("fast") forms of the field routines, through the same dispatchers the kernels
 * call.  Per element i: operands a[i], b[i] (slot 0) and c[i], d[i] (slot 1; read but unused by the one-slot ops), up to four results
 * out[k*n + i] (k = 0..3, unused ones 0) and word[i]: bit 0 = this lane's own bit of the routine's `rare` mask (started at 0),
 * bit 1 = whether any lane of its wave raised it (0 for the exact ops).  The launch has 256 threads per workgroup with element i on
 * thread i, so a wave is the 64 consecutive elements 64w .. 64w+63; the last wave may be partial.  The value of a flagged lane is undefined.
 * op 0: mont_mul2 -> a*b*2^-128, c*d*2^-128 (a, c < 2^128; b, d < p)      1: fe_addsub2 -> a+b, a-b, c+d, c-d
 *    2: fe_add_fast -> a+b   3: fe_sub_fast -> a-b   4: mont_mul_fast -> a*b*2^-128
 *    5: mont_mul2_fast -> as op 0   6: fe_addsub2_fast -> as op 1   7: fe_neg -> -a
 * The self-repairing top-limb forms the batch kernel runs (always the canonical result, word[i] = 0; 8..15 are not codes):
 *   16: fe_add_fix -> a+b   17: fe_sub_fix -> a-b   18: mont_mul_fix -> a*b*2^-128
 *   19: mont_mul2_fix -> as op 0   20: fe_addsub2_fix -> as op 1 */
int sc_field_selftest2(int op, const void* a, const void* b, const void* c, const void* d, void* out, uint32_t* word, uint64_t n);

/* ---- device vectors ----------------------------------------------------------------------- */
int sc_vec_alloc(uint64_t n, sc_vec_t** out);
int sc_vec_free(sc_vec_t* v);
/* a handle over device memory the CALLER owns (n field elements at d_elems, e.g. a torch tensor's storage): no copy; the memory must
 * outlive the handle and every call enqueued with it; sc_vec_free releases the handle only */
int sc_vec_wrap(void* d_elems, uint64_t n, sc_vec_t** out);
uint64_t sc_vec_len(const sc_vec_t* v);
void* sc_vec_ptr(sc_vec_t* v);         /* raw device pointer */
int sc_vec_zero(sc_vec_t* v);                                   /* all elements = 0 (library stream) */
int sc_vec_upload(sc_vec_t* v, uint64_t offset, const void* host, uint64_t count);
int sc_vec_download(const sc_vec_t* v, uint64_t offset, void* host, uint64_t count);
int sc_vec_gather(const sc_vec_t* v, const uint64_t* indices, uint64_t k, void* host_out); /* host_out[i] = v[indices[i]] */
/* `count` elements device to device, asynchronous on `stream` (a library vector <-> caller-owned device memory, e.g. a torch tensor) */
int sc_memcpy_dev(void* d_dst, const void* d_src, uint64_t count, void* stream);

/* ---- ntt / intt : code/ntt.py:3-18, :20-30 -------------------------------------------------- */
/* out[i] = sum_j in[j] * root^(i*j); inverse != 0: uses root^-1 and scales by n^-1 (ntt.py:27-30).
 * n must be a power of two (n <= 1 copies).  root is validated like ntt.py:10-11.
 * _dev: enqueued on `stream` (NULL: the library's).  Transforms -- this entry and sc_coset_evaluate_dev -- may be IN FLIGHT ON SEVERAL
 * STREAMS AT ONCE (independent columns side by side: each stream has its own intermediate vector); at 2^20 two streams carry
 * 1.4 x the elements per second of one.  Every other entry keeps the one-stream-at-a-time rule of its scratch buffers. */
int sc_ntt(const void* in, void* out, uint64_t n, const uint64_t root[2], int inverse);
int sc_ntt_dev(const void* d_in, void* d_out, uint64_t n, const uint64_t root[2], int inverse, void* stream);
/* The same transform for `cols` independent vectors of length n -- the registers of a trace, the loops over columns of
 * code/fast_stark.py:84-90 and :100-104 -- column c at element c * n of d_in and of d_out (d_in == d_out is allowed): one set of
 * launches covers up to 2^26 elements (64 columns of 2^20), every pass over cols x its tiles, so the workgroups of one column start
 * while those of another finish, and the 2^12-element tiles of a batch run two workgroups per CU (a lone 2^20 transform is one
 * workgroup per CU with every CU in the same phase: 30 G elements/s; 16-64 columns: 43-44; 64 columns of 2^16: 45-49 against 3.4
 * one at a time -- DESIGN.md 3.1).
 * The eight-element kernels correct by +-p on the top and bottom 32-bit limbs only; where the carry between them matters
 * (probability 2^-32 per lane and operation on the values a transform carries after its first twiddles) the operation ripples it
 * through the middle limbs on the spot, behind a wave-uniform branch, so every stored value is the canonical one and a pass is one
 * launch.  sc_set_tuning("fast_fixups", 0) runs the exact four-limb corrections on every tile instead; results are the same bits
 * either way. */
int sc_ntt_columns_dev(const void* d_in, void* d_out, uint64_t n, uint64_t cols, const uint64_t root[2], int inverse, void* stream);

/* ---- building blocks of the multi-GPU four-step NTT (no reference counterpart: the reference is single-process;
 *      together they compute exactly ntt.py:3-18 on a domain sharded over ranks, see stark-anatomy_amd/sharded.py) */
/* kind 0: d_in [len][batch] row-major, transform along axis 0 for every column, same layout out (natural order).
 * kind 1: d_in [batch][len], transform every row, output TRANSPOSED d_out [len][batch].  root: primitive len-th root. */
int sc_ntt_batch_dev(const void* d_in, void* d_out, uint64_t len, uint64_t batch, int kind, const uint64_t root[2], void* stream);
/* the same with the two fusions the sharded transform uses: kind 0 may multiply output (row r, column c) by
 * outer_root^(r * (outer_col_base + c)) [* outer_order^-1 if outer_scale_ninv] in its store epilogue (outer_root NULL = off);
 * kind 1 may read its input as [chunks][batch][len/chunks] (the layout all_to_all_single delivers) instead of [batch][len]. */
int sc_ntt_batch_ex_dev(const void* d_in, void* d_out, uint64_t len, uint64_t batch, int kind, const uint64_t root[2],
                        const uint64_t outer_root[2], uint64_t outer_order, uint64_t outer_col_base, int outer_scale_ninv, uint64_t chunks, void* stream);
/* kind 1 for ONE ROW BLOCK of the corner turn (overlap of the all-to-all with the row stage): transforms `batch` rows given as
 * [chunks][batch][len/chunks] and writes them as `batch` adjacent columns of a wider transposed output [len][out_ld]
 * (d_out points at the block's first column). */
int sc_ntt_rows_t_ld_dev(const void* d_in, void* d_out, uint64_t len, uint64_t batch, const uint64_t root[2], uint64_t chunks, uint64_t out_ld, void* stream);
/* The sharded transform as one plan object per rank (what SURVEY.md 8(b) sketched as `sc_ntt_sharded`): computes exactly
 * ntt.py:3-18 (inverse: ntt.py:20-30) of a length-2^log2n vector partitioned over `world` ranks.  n = n1 * n2 (n1 = 2^8 above
 * 2^16, else the square split); rank g holds the column slab [R][C/G] of the row-major R x C matrix of its input (forward: R = n1,
 * C = n2; inverse: R = n2, C = n1) and receives the column slab [C][R/G] of the output (sc_fourstep_shape returns R and C).
 * `d_send` and `d_recv` are caller-owned buffers of n/G elements laid out [G][R/G][C/G].  All entries are asynchronous on `stream`.
 *   sc_fourstep_cols_dev : column transforms + outer twiddle (+ n^-1 for the inverse), d_src -> d_send; block h of d_send is what
 *       rank h must receive into block g of ITS d_recv.  With d_recv_diag != NULL the block the rank keeps (h == g) is written
 *       straight into d_recv_diag (= the rank's d_recv) and the matching block of d_send is left untouched: it is never
 *       copied or sent.
 *   sc_fourstep_rows_dev : row transforms of the rank's rows [block * R/(G nblocks), ...) (nblocks = 1: all of them) read in
 *       place from d_recv, written transposed into d_dst [C][R/G].  defer_last_pass != 0 with a two-pass row transform runs
 *       only the first pass here; sc_fourstep_rows_finish_dev then runs the second pass for ALL rows in one launch (and is a
 *       no-op when nothing was deferred).
 *   sc_fourstep_run_dev : the whole transform, with the corner turn issued over the library's own RCCL communicator
 *       (sc_comm_init; grouped ncclSend/ncclRecv to the G - 1 peers, straight from d_send into the peers' d_recv).  nblocks > 1
 *       issues the exchange as row blocks on the library's communication stream and starts the row transforms of a block as
 *       soon as it has landed.  force_diag_exchange (tests): the rank's own block goes through RCCL too. */
typedef struct sc_fourstep sc_fourstep_t;
typedef struct { char internal[128]; } sc_rccl_id_t;   /* = ncclUniqueId */
int sc_fourstep_create(int log2n, const uint64_t root[2], int rank, int world, sc_fourstep_t** plan);
/* the same with the split chosen by the caller: n1 = 2^log_n1 (0 = the default: 2^8 above 2^16, square below) */
int sc_fourstep_create_ex(int log2n, const uint64_t root[2], int rank, int world, int log_n1, sc_fourstep_t** plan);
int sc_fourstep_free(sc_fourstep_t* plan);
int sc_fourstep_shape(const sc_fourstep_t* plan, int inverse, uint64_t* rows, uint64_t* cols_total);
int sc_fourstep_cols_dev(const sc_fourstep_t* plan, int inverse, const void* d_src, void* d_send, void* d_recv_diag, void* stream);
int sc_fourstep_rows_dev(const sc_fourstep_t* plan, int inverse, const void* d_recv, void* d_dst, uint64_t block, uint64_t nblocks, int defer_last_pass, void* stream);
int sc_fourstep_rows_finish_dev(const sc_fourstep_t* plan, int inverse, void* d_dst, void* stream);
/* the library's RCCL communicator (one per process; RCCL is dlopen'ed: rccl_path NULL = the copy already in the process, e.g.
 * torch's, else librccl.so.1): rank 0 makes an id, the launcher distributes its 128 bytes (torch.distributed broadcast), every rank
 * calls sc_comm_init with it (collective, blocking).  SC_ERR_UNSUPPORTED without RCCL. */
int sc_comm_unique_id(const char* rccl_path, sc_rccl_id_t* id_out);
int sc_comm_init(const char* rccl_path, const sc_rccl_id_t* id, int rank, int world);
int sc_comm_destroy(void);
int sc_fourstep_run_dev(const sc_fourstep_t* plan, int inverse, const void* d_src, void* d_send, void* d_recv, void* d_dst, uint64_t nblocks, int defer_last_pass,
                        int force_diag_exchange, void* stream);
/* DIRECT-STORE corner turn: no collective at all.  Every rank owns a REGION of device memory -- [4 KiB of flags][receive buffer
 * 0][receive buffer 1], sc_fourstep_region_bytes() bytes -- exported with a HIP IPC handle (64 bytes, carried to the other ranks
 * by the caller's launcher) and mapped by every peer (sc_ipc_region_open).  sc_fourstep_run_direct_dev then runs the whole
 * transform: the column stage stores block h of its output STRAIGHT INTO rank h's receive buffer (the stores cross xGMI; no
 * send buffer, no copy kernel, one HBM write + read per element less than a send/recv exchange), a one-wave kernel raises this
 * rank's flag at every peer and waits for theirs (system-scope atomics), and the row stage reads the rank's own receive buffer.
 * Consecutive transforms alternate between the two receive buffers, so a peer's next column stage never overwrites what a row
 * stage is still reading.  Every rank must run the same transforms in the same order.  A barrier that waits ~2 s for a peer
 * gives up and writes the transform's number to a pinned word of the plan: that transform's output is undefined, and from then on
 * the failure is STICKY -- sc_fourstep_direct_status reports the number (no copy, no wait) and every later
 * sc_fourstep_run_direct_dev returns SC_ERR_TIMEOUT until sc_fourstep_set_peers is called again (the peers' buffers are out of
 * step; the caller re-creates the set-up or goes back to the collective exchange).
 * The region is FINE-GRAINED device memory (hipExtMallocWithFlags, as RCCL's peer-written buffers are): peers write into it
 * while this GPU's kernels poll and read it.  sc_ipc_region_create_ex chooses: kind 1 fine-grained (coarse-grained when the
 * runtime cannot export one), 0 coarse-grained = plain hipMalloc, -1 the default (fine-grained unless STARKCORE_IPC_COARSE=1);
 * sc_ipc_region_kind: 1 fine-grained, 0 coarse-grained, -1 no region created yet. */
int sc_ipc_region_create(uint64_t bytes, void** d_region, uint8_t handle_out[64]);
int sc_ipc_region_create_ex(uint64_t bytes, int kind, void** d_region, uint8_t handle_out[64]);
int sc_ipc_region_kind(int* fine_grained);
int sc_ipc_region_open(const uint8_t handle[64], void** d_region);
int sc_ipc_region_close(void* d_region);        /* a region opened from a peer's handle */
int sc_ipc_region_free(void* d_region);         /* a region this process created */
int sc_fourstep_region_bytes(const sc_fourstep_t* plan, uint64_t* bytes);
int sc_fourstep_set_peers(sc_fourstep_t* plan, void* const* regions);      /* regions[h]: rank h's region as mapped HERE (own: its own) */
int sc_fourstep_run_direct_dev(sc_fourstep_t* plan, int inverse, const void* d_src, void* d_dst, void* stream);
int sc_fourstep_direct_status(const sc_fourstep_t* plan, uint64_t* timed_out_epoch);
/* d_data[r][c] *= root^((row_base + r) * (col_base + c)) * scale, root of order `order` (scale may be NULL = 1);
 * cols a power of two, every exponent below `order`.  rows == 0 or cols == 0: SC_OK, nothing happens, nothing else is looked at. */
int sc_twiddle_matrix_dev(void* d_data, uint64_t rows, uint64_t cols, uint64_t row_base, uint64_t col_base, const uint64_t root[2], uint64_t order,
                          const uint64_t scale[2], void* stream);

/* ---- fast_coset_evaluate : code/ntt.py:132-135 (Polynomial.scale univariate.py:153-154 fused) -- */
/* out[i] = sum_{j<m} coeffs[j] * (offset * generator^i)^j, i < order; m <= order. */
int sc_coset_evaluate(const void* coeffs, uint64_t m, const uint64_t offset[2], const uint64_t generator[2], uint64_t order, void* out);
int sc_coset_evaluate_dev(const void* d_coeffs, uint64_t m, const uint64_t offset[2], const uint64_t generator[2], uint64_t order, void* d_out, void* stream);
/* The same for `cols` polynomials of m >= 1 coefficients each -- the loop over registers of code/fast_stark.py:100-104 -- polynomial c at
 * element c * m of d_coeffs, its values at element c * order of d_out; one set of launches (sc_ntt_columns_dev). */
int sc_coset_evaluate_columns_dev(const void* d_coeffs, uint64_t m, uint64_t cols, const uint64_t offset[2], const uint64_t generator[2], uint64_t order, void* d_out, void* stream);

/* ---- NTT core of fast_multiply : code/ntt.py:51-64 ----------------------------------------- */
/* out[0..n_out) = intt(root, ntt(root, a||0) * ntt(root, b||0))[0..n_out); na, nb, n_out <= order.
 * (the degree bookkeeping / order halving of ntt.py:38-49 stays in the host shim.) */
int sc_poly_mul(const void* a, uint64_t na, const void* b, uint64_t nb, const uint64_t root[2], uint64_t order, void* out, uint64_t n_out);

/* ---- NTT core of fast_coset_divide : code/ntt.py:159-176 ----------------------------------- */
/* out[0..n_out) = unscale( intt( ntt(scale(a)) / ntt(scale(b)) ) ); SC_ERR_DIV_ZERO if a divisor value is 0 */
int sc_coset_divide(const void* a, uint64_t na, const void* b, uint64_t nb, const uint64_t offset[2], const uint64_t root[2], uint64_t order, void* out, uint64_t n_out);
/* the same on coefficient vectors in HBM (d_out: n_out coefficients).  *exact (may be NULL; makes the call synchronous) is set to 1
 * iff the interpolant's coefficients [n_out, order) all vanish: with order > deg(a), exactly the condition "b divides a and the
 * quotient has fewer than n_out coefficients" that Polynomial.__truediv__ asserts (code/univariate.py:99-103) */
int sc_coset_divide_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, const uint64_t offset[2], const uint64_t root[2], uint64_t order,
                        void* d_out, uint64_t n_out, int* exact, void* stream);
/* The same division, and the pointwise division of code/ntt.py:172 on its own, with NOTHING waited for: what the reference asserts on
 * the spot -- "divide by zero" (code/algebra.py:92) and, for the coset division, a zero remainder (code/univariate.py:99-103) -- is
 * decided on the device and arrives in *later behind the work; sc_later_wait returns words_out[0] != 0: a divisor value was zero;
 * words_out[1]: the highest index, counted from n_out, of a non-zero coefficient of the interpolant above the quotient, -1 iff the
 * division is exact (always -1 for the pointwise form).  A prover collects its checks where it has to wait anyway (before the next
 * Fiat-Shamir challenge) instead of idling the GPU at every division.  sc_later_wait frees the handle (it is also how one is abandoned).
 * SC_ERR_UNSUPPORTED: no pinned slot free (they are shared with the asynchronous Merkle roots); NOTHING was enqueued, so d_out -- and a
 * numerator divided in place -- is as it was: use the waiting forms.  Each check has device words of its own, so checks in flight on
 * any number of streams do not disturb one another; but the coset form, like sc_coset_divide_dev, runs its transforms in the
 * library's shared scratch, so coset divisions (deferred or not) must be ordered on one stream.  The pointwise form has no such limit. */
int sc_coset_divide_later_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, const uint64_t offset[2], const uint64_t root[2], uint64_t order,
                              void* d_out, uint64_t n_out, sc_later_t** later, void* stream);
int sc_pointwise_div_later_dev(const void* d_a, const void* d_b, void* d_out, uint64_t n, sc_later_t** later, void* stream);
int sc_later_wait(sc_later_t* later, int64_t words_out[8]);
/* The two deferred divisions for `cols` COLUMNS of one matrix at once (column c at element c * ld of its operand), with ONE verdict:
 * whatever `cols`, the call reserves exactly one pinned slot, before anything is enqueued (SC_ERR_UNSUPPORTED: none free, nothing
 * enqueued, every operand as it was).  Pointwise form: out[c][i] = a[c][i] / b[c][i], i < n; ld_b == 0: ONE divisor row shared by all
 * columns, inverted once per chunk of columns instead of once per column (sc_set_tuning("div_cols_chunk")); d_out may be d_a
 * (in place) only with ld_out == ld_a: one matrix with two strides is SC_ERR_BAD_ARG; operands that overlap in any other way are not allowed.
 * Coset form: column c's quotient is the first n_out[c] coefficients (n_out: host array of `cols` entries) of the interpolant
 * sc_coset_divide_dev computes for (a_c, b_c) -- a_c: na coefficients, b_c: nb coefficients (a shorter divisor is zero-padded by the
 * caller), ld_b == 0: one divisor, evaluated once -- and the exactness scan of column c covers [n_out[c], order).
 * sc_later_wait then returns words_out[2]: the LOWEST column that met a zero divisor or left a remainder, -1 if none; words_out[0],
 * words_out[1]: that column's zero-divisor flag and remainder index, counted from its n_out[c] -- (0, -1) if no column failed, so the
 * words keep the meaning they have for a single division; words_out[3]: the number of failing columns.  Quotient values are
 * unspecified where words_out[0] != 0.  The per-column device words and the value matrices are the call's own (returned to the
 * pool behind the streams in use), so there is no shared scratch and no one-stream rule: the operands must be complete on `stream`,
 * and columns-form calls on different streams do not disturb one another beyond sharing the table caches like every transform. */
int sc_pointwise_div_columns_later_dev(const void* d_a, uint64_t ld_a, const void* d_b, uint64_t ld_b /* 0: one shared row */,
                                       void* d_out, uint64_t ld_out, uint64_t n, uint64_t cols, sc_later_t** later, void* stream);
int sc_coset_divide_columns_later_dev(const void* d_a, uint64_t na, uint64_t ld_a, const void* d_b, uint64_t nb, uint64_t ld_b /* 0: shared */,
                                      uint64_t cols, const uint64_t offset[2], const uint64_t root[2], uint64_t order,
                                      void* d_out, const uint64_t* n_out /* host, cols entries */, uint64_t ld_out,
                                      sc_later_t** later, void* stream);
/* ---- division with remainder : code/univariate.py:80-97 (Polynomial.divide) ------------------- */
/* a = q * b + r for a of na and b of nb coefficients, b[nb-1] != 0 and na >= nb >= 1: q gets na - nb + 1 coefficients (zero on top
 * where a's top coefficients are zero), r gets nb - 1.  No coset, no transform order to pass, any divisor -- monic or not, with roots
 * anywhere: rev(b) is inverted as a power series by Newton doubling, rev(q) = rev(a) * rev(b)^-1 mod y^(na-nb+1), and r = a - q * b
 * is formed cyclically at the divisor's size (csrc/polydiv.cuh).  q == NULL: no quotient is stored; r == NULL: no remainder is
 * computed (that step is skipped); both NULL: SC_ERR_BAD_ARG.  nb == 1 divides by the constant (r has no coefficients).
 * SC_ERR_BAD_ARG, before anything is enqueued: nb == 0, na < nb, na > 2^31, a pitch below what is stored per column, outputs that
 * overlap an operand or each other.  SC_ERR_DIV_ZERO: b[nb-1] == 0 (the one value the call reads back, before any work is enqueued:
 * nothing is written to q or r).  The host form is synchronous; the _dev forms wait for that one value and enqueue the rest. */
int sc_poly_divmod(const void* a, uint64_t na, const void* b, uint64_t nb, void* q /* na-nb+1 */, void* r /* nb-1 */);
int sc_poly_divmod_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, void* d_q, void* d_r, void* stream);
/* The same for `cols` numerators that are columns of one matrix (column c: na coefficients at element c * ld_a) and ONE divisor: the
 * series and the divisor's transform are computed once, every transform and every kernel runs once per set of columns
 * (sc_set_tuning("div_cols_launch_log") values per set).  Column c's na - nb + 1 quotient coefficients go to element c * ld_q of d_q,
 * its nb - 1 remainder coefficients to element c * ld_r of d_r; nothing between the columns is written.  cols == 0: SC_OK, nothing
 * happens.  The temporaries are the call's own (returned to the pool behind the streams in use): no shared scratch, no one-stream rule. */
int sc_poly_divmod_columns_dev(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols,
                               const void* d_b, uint64_t nb,            /* ONE divisor for all columns */
                               void* d_q, uint64_t ld_q, void* d_r, uint64_t ld_r, void* stream);
/* ---- products, powers, products of many : code/univariate.py:48-57 (__mul__), :140-150 (__xor__) -- */
/* Operands and results resident in HBM.  The library picks the transform itself: the smallest power of two that holds the result, with
 * the root Field.primitive_nth_root gives -- no root, no order to pass.  The length passed in is the length used: zero coefficients on
 * top are allowed, so are all-zero operands, and the WHOLE stated output length is written (zero on top where the operands' top
 * coefficients are zero) -- the list length of the reference's product.  Nothing behind the stated output length is touched, nothing
 * between a row's length and its stride is read into a result or written (csrc/polymul.cuh).
 * SC_ERR_BAD_ARG, before anything is enqueued: a NULL pointer, a zero length, a stride below its length, an output that overlaps an
 * operand, a result of more than 2^32 coefficients.  Nothing is read back: every call is enqueued on `stream` and returns.
 * The temporaries are the call's own (returned to the pool behind the streams in use): no shared scratch, no one-stream rule -- the
 * operands must be complete on `stream`, and calls on different streams do not disturb one another beyond sharing the table caches
 * like every transform.  (The host entry sc_poly_mul above works in the shared scratch and is bound to the one-stream rule.)
 * sc_poly_mul_dev: out = a * b, na + nb - 1 coefficients; d_a == d_b with na == nb (a square) is transformed once. */
int sc_poly_mul_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, void* d_out /* na+nb-1 */, void* stream);
/* out[c] = a[c] * b[c] for `cols` columns (column c of a matrix at element c * its stride); ld_b == 0: ONE multiplicand for all columns,
 * transformed once per call.  Every other transform and kernel runs once per set of columns (sc_set_tuning("div_cols_launch_log")
 * values per set, at most 65 535 columns); the multiplicands are read at their strides, not copied.  cols == 0: SC_OK, nothing happens. */
int sc_poly_mul_columns_dev(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols,
                            const void* d_b, uint64_t nb, uint64_t ld_b /* 0: one shared multiplicand */,
                            void* d_out, uint64_t ld_out, void* stream);
/* out = a^exponent, exponent * (na - 1) + 1 coefficients: exponent 0 gives the single coefficient 1 (also for an all-zero a), exponent 1
 * a copy, anything else one forward transform at the result's size, one pointwise power and one inverse transform. */
int sc_poly_pow_dev(const void* d_a, uint64_t na, uint64_t exponent, void* d_out /* exponent*(na-1)+1 */, void* stream);
/* out = the product of `count` rows of n coefficients each (row j at element j * ld of d_rows), count * (n - 1) + 1 coefficients: a
 * balanced tree of log2(count) levels, every level one columns transform of all its rows, the pairwise products and one inverse
 * columns transform per set of rows (sets as above); an odd last row is carried up.  count == 1 copies; count == 0: SC_OK, nothing happens. */
int sc_poly_product_dev(const void* d_rows, uint64_t n, uint64_t ld, uint64_t count, void* d_out /* count*(n-1)+1 */, void* stream);
/* ---- values at points, directly : code/univariate.py:99-105 (evaluate, evaluate_domain) ------- */
/* out[c * ld_out + j] = sum_i coeffs[c * ld_in + i] * points[j]^i,  i < m, j < k, c < cols: `cols` polynomials of m coefficients each
 * (column c at element c * ld_in of d_coeffs) at the SAME k points, all resident in HBM.  The work is m * k * cols modular products --
 * no tree, no transform: the route for few points against many coefficients (one point included), where sc_polytree_evaluate_columns_dev
 * would first reduce the polynomial modulo a zerofier at the polynomial's own size (csrc/polyeval.cuh).  Values are canonical residues
 * in and out; points may repeat and need not be distinct from one another or from 0.  m == 0 gives zeros; k == 0 or cols == 0: SC_OK,
 * nothing is enqueued.  Nothing between a column's k results and the next stride is written, nothing between a column's m coefficients
 * and the next stride is read into a result.
 * SC_ERR_BAD_ARG, before anything is enqueued: a NULL pointer with a non-zero count, ld_in < m or ld_out < k with cols > 1, m > 2^32,
 * k * cols > 2^32, an output range that overlaps the coefficients or the points.
 * The coefficients are cut into chunks of at least 2^"eval_chunk_log" (sc_set_tuning) coefficients; a first launch computes every
 * chunk's own value -- coefficients across the lanes of a workgroup for fewer than "eval_points_across_min" points and for calls too small
 * to fill the device, points across lanes otherwise -- and a second, small launch combines the chunks (skipped when there is one).  No workgroup waits for another and no
 * atomics touch field elements: the results are exact and the same for every chunk length, form and schedule.
 * The _dev form reads nothing back and only ENQUEUES on `stream` (NULL: the library stream).  Its temporaries are the call's own
 * (returned to the pool behind the streams in use): no shared scratch, no one-stream rule -- the operands must be complete on
 * `stream`, and calls on different streams do not disturb one another.  The host form takes host buffers and one column, works on the
 * library stream and is synchronous. */
int sc_poly_eval_points_dev(const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols,
                            const void* d_points, uint64_t k, void* d_out, uint64_t ld_out, void* stream);
int sc_poly_eval_points(const void* coeffs, uint64_t m, const void* points, uint64_t k, void* out /* k values */);
/* Polynomial.degree (code/univariate.py:7-17) of a coefficient vector in HBM: index of the last non-zero entry, -1 if none (synchronous) */
int sc_vec_degree_dev(const void* d_v, uint64_t n, int64_t* degree_out, void* stream);
/* The same for `cols` vectors of n entries each, column c at element c * ld of d_v (ld >= n; entries between the columns are not
 * read): degrees_out[c] as above.  One kernel and one host wait for up to 4 096 columns (synchronous; cols == 0: nothing happens). */
int sc_vec_degree_columns_dev(const void* d_v, uint64_t n, uint64_t ld, uint64_t cols, int64_t* degrees_out, void* stream);

/* ---- pointwise helpers (ntt.py:61, :172; univariate.py:153-154) ------------------------------ */
int sc_pointwise_mul_dev(const void* d_a, const void* d_b, void* d_out, uint64_t n, void* stream);
int sc_pointwise_div_dev(const void* d_a, const void* d_b, void* d_out, uint64_t n, void* stream); /* sync; SC_ERR_DIV_ZERO */
int sc_scale_dev(const void* d_in, void* d_out, uint64_t n, const uint64_t factor[2], void* stream); /* out[i] = in[i] * factor^i */
/* (factor is a canonical residue: factor >= p is SC_ERR_BAD_ARG with nothing written, as in sc_scale_columns_dev; n == 0: nothing happens) */
/* acc[shift + j] += weight * src[j], j < n_src: one term `Polynomial([weight]) * (x ^ shift) * term` of the nonlinear combination
 * of code/fast_stark.py:130-145 on coefficient vectors in HBM (shift + n_src <= n_acc) */
int sc_axpy_shift_dev(void* d_acc, uint64_t n_acc, const void* d_src, uint64_t n_src, uint64_t shift, const uint64_t weight[2], void* stream);
/* The whole combination in ONE pass: out[c][i] = sum_t weights[c][t] * src_t[c][i - shift_t] over the terms with
 * shift_t <= i < shift_t + n_t, for i < n_out and c < cols (term t's column c at element c * ld of d_src; out's at c * ld_out).  Every
 * element of [0, n_out) of every column is written once -- zero where no term covers it -- so d_out needs no zeroing and may not
 * alias a source (SC_ERR_BAD_ARG).  weights: host, [cols][nterms], canonical; shift + n <= n_out; any nterms >= 1; cols == 0 or
 * n_out == 0: nothing happens.  Equal to the chain of sc_axpy_shift_dev calls over a zeroed accumulator, column by column. */
typedef struct { const void* d_src; uint64_t ld; uint64_t n; uint64_t shift; } sc_combine_term_t;
int sc_combine_columns_dev(const sc_combine_term_t* terms, uint64_t nterms, const void* weights /* host [cols][nterms] canonical */,
                           uint64_t cols, void* d_out, uint64_t n_out, uint64_t ld_out, void* stream);
/* the same scaling (univariate.py:153-154) on one rank's column slab [rows][cols] of a vector viewed as a rows x row_len
 * matrix (multi-GPU fast_coset_evaluate / fast_coset_divide, ntt.py:132-135, :159-176):
 * out[r][c] = in[r][c] * factor^(r * row_len + col_base + c); cols a power of two, col_base + cols <= row_len.
 * factor is a canonical residue: factor >= p is SC_ERR_BAD_ARG with nothing written.  rows == 0 or cols == 0: nothing happens. */
int sc_scale_slab_dev(const void* d_in, void* d_out, uint64_t rows, uint64_t cols, uint64_t row_len, uint64_t col_base, const uint64_t factor[2], void* stream);

/* ---- fast_zerofier / fast_evaluate / fast_interpolate : code/ntt.py:66-80, :82-100, :102-130 -- */
/* The reference recurses node by node (split at len//2, schoolbook remainders, zerofiers recomputed per node); zerofier,
 * values and interpolant are unique, so the device works level by level on a perfect tree over the k points padded with zeros
 * to a power of two (stark-anatomy_amd/csrc/polytree.cuh).  Points are arbitrary canonical residues; they need to be distinct
 * only for interpolation (a repeated point gives SC_ERR_DIV_ZERO, like the assertion of algebra.py:92 in ntt.py:124-125).
 * The transforms use the field's own 2^j-th roots (algebra.py:104-111); no root argument is needed. */
int sc_zerofier(const void* points, uint64_t k, void* out);                                   /* out: k + 1 coefficients of prod (X - d_i) */
int sc_evaluate(const void* coeffs, uint64_t m, const void* points, uint64_t k, void* out);   /* out[i] = poly(points[i]), any m */
int sc_interpolate(const void* points, const void* values, uint64_t k, void* out);            /* out: k coefficients (degree < k) */
/* the same on device pointers with the tree kept between calls (one tree serves any number of evaluations / interpolations).
 * sc_polytree_build / sc_polytree_build_dev take 1 <= k <= 2^30 points (SC_ERR_BAD_ARG for k == 0, SC_ERR_UNSUPPORTED above 2^30);
 * the tree pads them to K = the power of two >= k leaves and keeps about 3 * K * log2(K) elements. */
int sc_polytree_build(const void* points, uint64_t k, sc_polytree_t** tree);                  /* k >= 1 */
int sc_polytree_build_dev(const void* d_points, uint64_t k, sc_polytree_t** tree, void* stream);
uint64_t sc_polytree_points(const sc_polytree_t* tree);
int sc_polytree_zerofier_dev(const sc_polytree_t* tree, void* d_out, void* stream);           /* k + 1 coefficients */
/* d_points: the tree's points again, only read when m exceeds the padded domain size (chunked evaluation); may be NULL otherwise */
int sc_polytree_evaluate_dev(sc_polytree_t* tree, const void* d_coeffs, uint64_t m, const void* d_points, void* d_out, void* stream);
int sc_polytree_interpolate_dev(sc_polytree_t* tree, const void* d_values, void* d_out, void* stream);
/* The same two for `cols` polynomials in one call: column c's m coefficients (k values) start at element c * ld_in of the input, its
 * k results go to element c * ld_out of d_out; elements between a column's end and the next pitch are neither read nor written.  m
 * is common to the call (shorter polynomials are zero-padded by the caller; m == 0 gives zeros).  The results are those of `cols`
 * calls of the single entries, bit for bit.  A set of C' = 2^j columns goes through the tree with the column index innermost (a level
 * is [2^l][K >> l][C'], K the power of two >= k), so every step -- the batched transforms of a level, the elementwise kernels -- is
 * issued once per set; a set's temporaries hold 2K * C' elements, at most 2^26 (sc_set_tuning "tree_cols_launch_log"); more columns go set
 * after set, a last set of fewer columns is padded to the next power of two with lanes of zeros that are never stored.  Interpolation
 * keeps 1 / Z'(d_i) in the tree (built by the first call, which waits for it: a repeated point is SC_ERR_DIV_ZERO "divide by zero", and
 * nothing is kept); evaluation builds the tree's inverse series on first use as the single entry does.  Apart from those first-use
 * builds the calls only ENQUEUE on `stream`: results are valid in stream order, temporaries are returned behind the stream.
 * d_points is read only when m > K (NULL there: SC_ERR_BAD_ARG).  cols == 0: SC_OK, nothing enqueued; with cols > 1 a pitch below the
 * column's length (ld_in < m, ld_in < k, ld_out < k): SC_ERR_BAD_ARG.  d_out may NOT overlap the input. */
int sc_polytree_evaluate_columns_dev(sc_polytree_t* tree, const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const void* d_points, void* d_out, uint64_t ld_out, void* stream);
int sc_polytree_interpolate_columns_dev(sc_polytree_t* tree, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream);
/* Polynomial.interpolate_domain (code/univariate.py:107-121) for ANY points: the columns interpolation above with the weights
 * inv0(Z'(d_i)) in place of 1 / Z'(d_i), where inv0 is the reference's Field.inverse (code/algebra.py:87-89), which maps 0 to 0.  The
 * result is  sum_i v_i * inv0(Z'(d_i)) * Z(X) / (X - d_i)  with Z the zerofier of all points with their multiplicities: a repeated
 * point (Z' = 0 there) drops its own terms and nothing fails; always k coefficients.  For distinct points the coefficients equal
 * sc_polytree_interpolate_columns_dev's bit for bit.  The tree keeps this weight table beside the other one (one extra kernel, built by
 * the first call; it IS the other table where that exists, since that was built without a zero derivative).  The existing entries
 * keep their behaviour on a tree this entry has used: a repeated point is still SC_ERR_DIV_ZERO from sc_polytree_interpolate_dev and
 * sc_polytree_interpolate_columns_dev, and nothing of theirs is kept.  Strides, overlap, sets of columns, cols == 0 and the
 * SC_ERR_BAD_ARG cases: as sc_polytree_interpolate_columns_dev.  Only enqueues (the tree's inverse series is built on first use, which
 * waits).  The weight table is built by the FIRST call, on that call's stream, and is not waited for: like every entry that takes a tree,
 * calls on one tree belong on one stream, or the first call's stream is ordered before whoever uses the tree next.  The progression tables need no such entry: their points are distinct by construction.
 * sc_interpolate_lagrange: host buffers, one column, k >= 1, k coefficients out, synchronous. */
int sc_polytree_interpolate_lagrange_columns_dev(sc_polytree_t* tree, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream);
int sc_interpolate_lagrange(const void* points, const void* values, uint64_t k, void* out);
int sc_polytree_free(sc_polytree_t* tree);

/* ---- the same three functions on a GEOMETRIC PROGRESSION  x_i = first * ratio^i, i < n : code/ntt.py:66-130 as called by
 * code/fast_stark.py:84-90 (the trace domain {omicron^i}) and :37 (the transition zerofier's domain) -----------------------
 * Zerofier, values and interpolant are unique, so on such a domain they are computed with O(1) transforms of length
 * M = pow2 >= 2n - 1 (Bluestein / Bostan-Schost) instead of a tree: same outputs as sc_polytree_* / the reference's recursion.
 * create: n >= 2, distinct points required (SC_ERR_UNSUPPORTED otherwise: use the tree, which reproduces the reference's
 * behaviour for repeated points).  Accepted are 2 <= n with 2n - 1 <= 2^28 (M <= 2^28, so n <= 2^27), first and ratio non-zero
 * residues below p, and ord(ratio) >= n: the full subgroup n = ord(ratio) is a progression, n = ord(ratio) + 1 repeats its first
 * point.  Everything else is SC_ERR_UNSUPPORTED with *domain untouched and nothing kept.  The *_dev calls only ENQUEUE on `stream` (NULL: the library stream): results are valid in
 * stream order; nothing waits, temporaries are returned behind the stream.
 * detect: is d_points[i+1] == d_points[i] * ratio for all i (ratio = points[1] / points[0])?  one small kernel + one sync. */
int sc_geodomain_create(const uint64_t first[2], const uint64_t ratio[2], uint64_t n, sc_geodomain_t** domain, void* stream);
uint64_t sc_geodomain_points(const sc_geodomain_t* domain);
int sc_geodomain_detect_dev(const void* d_points, uint64_t n, uint64_t first[2], uint64_t ratio[2], int* is_geometric, void* stream);
int sc_geodomain_zerofier_dev(const sc_geodomain_t* domain, void* d_out, void* stream);          /* n + 1 coefficients */
int sc_geodomain_evaluate_dev(const sc_geodomain_t* domain, const void* d_coeffs, uint64_t m, void* d_out, void* stream);   /* n values, any m */
int sc_geodomain_interpolate_dev(const sc_geodomain_t* domain, const void* d_values, void* d_out, void* stream);            /* n coefficients */
/* The same for `cols` columns in one set of launches: column c's n values start at element c * ld_in of d_values, its n coefficients
 * go to element c * ld_out of d_out (both strides >= n; elements of d_out between the columns are left alone).  The coefficients are
 * those of `cols` calls of sc_geodomain_interpolate_dev, bit for bit; every step -- four transforms, five elementwise kernels -- is
 * issued once for all columns (once per set of at most 2^26 / M and at most 65 536 columns, M the power of two >= 2n - 1).
 * d_out may NOT overlap d_values.  cols == 0: SC_OK, nothing enqueued; a null pointer or a stride below n: SC_ERR_BAD_ARG, nothing enqueued. */
int sc_geodomain_interpolate_columns_dev(const sc_geodomain_t* domain, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream);
/* Multipoint evaluation for `cols` polynomials of m coefficients each (any m; m == 0 gives zeros): column c's coefficients at element
 * c * ld_in of d_coeffs, its n values to element c * ld_out of d_out, those of sc_geodomain_evaluate_dev bit for bit.  The two transforms
 * and three elementwise kernels of an evaluation are issued once per set of columns (sets as above); m > n runs the same Horner over
 * chunks of n coefficients with the chunk powers shared by the columns.  Only enqueues.  cols == 0: SC_OK; with cols > 1, ld_in < m or
 * ld_out < n: SC_ERR_BAD_ARG.  d_out may NOT overlap d_coeffs. */
int sc_geodomain_evaluate_columns_dev(const sc_geodomain_t* domain, const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream);
int sc_geodomain_free(sc_geodomain_t* domain);

/* ---- MPolynomial.evaluate_symbolic in the value domain : code/multivariate.py:83-90 (call site fast_stark.py:109-110) ---- */
/* d_vals: [nvars][n] values of the point polynomials on an n-point domain (CONSUMED: converted in place to the library's
 * internal form); exps: host [nterms][nvars] exponents, coefs: host nterms packed residues.
 * d_out[i] = sum_t coefs[t] * prod_j vals[j][i]^exps[t][j].  With n > the degree of the result, an inverse NTT of d_out
 * gives exactly the polynomial the reference builds from schoolbook products (§8(f)-2). */
int sc_mpoly_eval_dev(void* d_vals, uint64_t nvars, uint64_t n, const uint8_t* exps, const void* coefs, uint64_t nterms, void* d_out, void* stream);
/* the same for several constraints over ONE set of point values: vals_converted != 0 says d_vals has been through an earlier call.
 * n may be any count (a rank's slab of a sharded value domain: the evaluation is pointwise). */
int sc_mpoly_eval_ex_dev(void* d_vals, uint64_t nvars, uint64_t n, const uint8_t* exps, const void* coefs, uint64_t nterms, void* d_out, int vals_converted, void* stream);
/* the same with variables that are TURNED copies of others (fast_stark.py:105-106: the point holds trace(X) and trace(omicron X); on
 * the coset g <omicron> the second one's codeword is the first one's, one place on): variable j is read as
 * d_vals[var_src[j]][(i + var_rot[j]) mod n] (n a power of two); var_src[j] == j with var_rot[j] == 0 for a variable stored in its
 * own place, var_src[j] == SC_MPOLY_ABSENT for one that no term uses (its place may hold anything and is not touched; a term that
 * does use it is an error).  A turned variable must point at a stored one.  var_src == var_rot == NULL: sc_mpoly_eval_ex_dev. */
#define SC_MPOLY_ABSENT 0xFFFFFFFFu
int sc_mpoly_eval_rot_dev(void* d_vals, uint64_t nvars, uint64_t n, const uint8_t* exps, const void* coefs, uint64_t nterms, void* d_out, int vals_converted,
                          const uint32_t* var_src, const uint64_t* var_rot, void* stream);

/* The same for `members` point sets over one n-point domain and `ncons` constraints in ONE launch (the AIR of a batch of proofs).
 * d_vals is only READ, in canonical form, and stays usable: nothing is converted in place.  Variable j of member m lies at element
 * var_base[j] + m * var_ld[j] of d_vals (host arrays of nvars <= 255 entries; var_ld[j] == 0: one row shared by all members, such as
 * the values of X; the trace variables are rows of the one matrix sc_coset_evaluate_columns_dev writes).  var_src / var_rot (both or
 * NULL) as above: a turned variable is read off a stored one of the same member, var_rot places on (n a power of two when anything
 * is turned, any count otherwise); SC_MPOLY_ABSENT: no term may use it.  Constraint c has nterms[c] terms (host array); exps holds the
 * constraints' [nterms[c]][nvars] exponent bytes one after the other, coefs their packed canonical coefficients likewise.
 * d_out[(m * ncons + c) * ld_out + i] = constraint c at point i of member m, canonical, ld_out >= n; a constraint of no terms gives
 * zeros.  Bit for bit what sc_mpoly_eval_rot_dev gives per member and constraint, from fewer products: each constraint is a Horner
 * walk in its variable of highest exponent (csrc/mpoly_plan.h).  Enqueued on `stream`.
 * members == 0 or ncons == 0: SC_OK, nothing happens.  SC_ERR_BAD_ARG (nothing enqueued): a null pointer, nvars 0 or above 255,
 * ld_out < n, an output that overlaps the values of a used variable, a coefficient not below p, a term that uses an absent variable, a
 * turned variable that does not point at a stored one; SC_ERR_NOT_POW2: turned variables with n not a power of two. */
int sc_mpoly_eval_columns_dev(const void* d_vals, uint64_t nvars, uint64_t n, uint64_t members, const uint64_t* var_base, const uint64_t* var_ld,
                              const uint32_t* var_src, const uint64_t* var_rot, uint64_t ncons, const uint64_t* nterms, const uint8_t* exps, const void* coefs,
                              void* d_out, uint64_t ld_out, void* stream);

/* Polynomial.scale (sc_scale_dev) for the rows of a matrix in one launch: d_out[c * ld_out + i] = d_in[c * ld_in + i] * factor^i, i < n,
 * c < cols (both strides >= n; elements between the rows are left alone; d_out may be d_in with the same stride: every element is
 * read by the thread that writes it.  No other overlap of the two matrices: it is not detected, and the result is undefined).  Bit for bit what
 * `cols` calls of sc_scale_dev give.  Enqueued on `stream`.  n == 0 or cols == 0: SC_OK, nothing happens; SC_ERR_BAD_ARG (nothing
 * enqueued): a null pointer, a stride below n, in place with another stride, a factor not below p. */
int sc_scale_columns_dev(const void* d_in, uint64_t ld_in, void* d_out, uint64_t ld_out, uint64_t n, uint64_t cols, const uint64_t factor[2], void* stream);

/* ---- Rescue-Prime : code/rescue_prime.py:25-60 (hash), :62-104 (trace) ----------------------- */
/* The permutation of the tutorial's hash over n inputs, one lane each.  In these two entries the state width is fixed: m = 2 (rate 1,
 * capacity 1), alpha = 3; the entries below them take any width.
 * d_in: n elements (reduced mod p on load).  params: HOST pointer to 4 + 4 * rounds packed canonical residues -- the MDS matrix
 * (row-major, 2 x 2), then the 2 m rounds round constants (round r: [4 r, 4 r + 2) after the cube, [4 r + 2, 4 r + 4) after the
 * inverse cube).  params is read for exactly 4 + 4 * rounds words: what lies behind them is neither read nor checked.
 * Enqueued on `stream`; n == 0 launches nothing.
 * hash:  d_out[k] = state[0] after `rounds` rounds (n elements).
 * trace: all rounds + 1 states, register s of input k's state t at d_out[(2 k + s) * (rounds + 1) + t] (2 n (rounds + 1) elements).
 * SC_ERR_BAD_ARG: rounds == 0 or > 27, a constant not below p, params NULL, or a NULL buffer with n > 0. */
int sc_rescue_prime_hash_dev(const void* d_in, uint64_t n, const void* params, uint64_t rounds, void* d_out, void* stream);
int sc_rescue_prime_trace_dev(const void* d_in, uint64_t n, const void* params, uint64_t rounds, void* d_out, void* stream);
/* The same permutation at any state width m = 2 .. 8 (alpha = 3), one lane per input, the state in registers.  Matrices are
 * COALESCED: register s of input k is element s * ld + k of its matrix, ld >= n.  params: HOST pointer to m * m + 2 * m * rounds
 * packed canonical residues -- the MDS matrix (row-major, m x m), then the round constants (round r: [2 r m, 2 r m + m) after the
 * cube, [2 r m + m, 2 (r + 1) m) after the inverse cube) -- read for exactly that many words during the call.  Every input word is
 * reduced mod p on load.  n == 0: SC_OK, nothing is launched.
 * permute:      d_out[s * ld_out + k] = register s of the permuted state of input k (m rows each).  d_out may be d_in with
 *               ld_out == ld_in (in place: every element is read by the lane that writes it).
 * sponge:       the state starts at zero; for each of `blocks` >= 1 blocks the message elements b * rate .. b * rate + rate - 1 of
 *               input k (element j at d_msg[j * ld_msg + k], blocks * rate rows) are added into registers 0 .. rate - 1, then the
 *               state is permuted; afterwards registers 0 .. out_len - 1 go to d_out[j * ld_out + k], 1 <= out_len <= rate,
 *               1 <= rate <= m - 1.  Padding is the caller's.  m = 2, rate = 1, blocks = 1, out_len = 1: sc_rescue_prime_hash_dev's
 *               result, bit for bit.
 * trace_states: all rounds + 1 states of n initial states (m rows of d_in), register s of input k's state t at
 *               d_out[(m * k + s) * (rounds + 1) + t] (m n (rounds + 1) elements): one input's registers are m adjacent columns.
 * SC_ERR_BAD_ARG, before anything is enqueued: m outside 2 .. 8, rate outside 1 .. m - 1, out_len outside 1 .. rate, blocks == 0,
 * rounds outside 1 .. 27, a constant not below p, params NULL, a NULL buffer with n > 0, a stride below n, an output that overlaps
 * an input (other than permute in place as above).
 * The calls only enqueue on `stream` and wait for nothing.  The constants travel as kernel arguments into a block of the call's own
 * (returned to the pool behind the streams in use): no shared scratch, no one-stream rule -- the operands must be complete on
 * `stream`, and calls on different streams do not disturb one another. */
int sc_rescue_prime_permute_dev(const void* d_in, uint64_t ld_in, void* d_out, uint64_t ld_out, uint64_t n, uint64_t m,
                                const void* params, uint64_t rounds, void* stream);
int sc_rescue_prime_sponge_dev(const void* d_msg, uint64_t ld_msg, uint64_t blocks, void* d_out, uint64_t ld_out, uint64_t out_len,
                               uint64_t n, uint64_t m, uint64_t rate, const void* params, uint64_t rounds, void* stream);
int sc_rescue_prime_trace_states_dev(const void* d_in, uint64_t ld_in, uint64_t n, uint64_t m, const void* params, uint64_t rounds,
                                     void* d_out, void* stream);

/* ---- Merkle trees over the Rescue-Prime sponge (csrc/rescue_merkle.cuh) ----------------------- */
/* A tree over the N rows (N a power of two, N >= 1) of a matrix, whose leaves and nodes are digests of digest_len = d field elements:
 *   leaf(row) = sponge(row, out_len = d),  node(left, right) = sponge(left + right, out_len = d)
 * with the sponge of the entries above at width m, rate 2 .. m - 1, 1 <= d <= rate, padded HERE (a single 1, then zeros up to a
 * multiple of the rate; never in memory): width / rate + 1 permutations per leaf, 2 d / rate + 1 per node.  No domain separation
 * between leaves and nodes.  Level j has N >> j nodes; node k of level j + 1 is node(level_j[2k], level_j[2k + 1]); a path's entry j is
 * node (index >> j) ^ 1 of level j (log2 N entries, the sibling leaf's digest first).  params: as above, a HOST pointer.
 * build_dev:  element j of row i at d_rows[j * ld + i], ld >= N (the `width` columns of a matrix of codewords, each contiguous, are
 *             the rows of the tree); every word is reduced mod p on load.  Only enqueues on `stream` -- one upload of the constants
 *             (kernel arguments, into a block of the call's own) and one launch per level -- and waits for nothing: no shared
 *             scratch, no one-stream rule; the rows must be complete on `stream`, and builds on different streams do not disturb one another.
 *             A level of at most sc_set_tuning("rescue_tree_split_max_nodes") nodes runs one lane per state REGISTER, a wider one
 *             one lane per node; the results are the same bits.
 * root:       waits for the build; digest_len canonical residues to the host.
 * open_batch: k paths in one launch; item t, level j, element e at paths_out[((t * log2 N) + j) * digest_len + e] (host, canonical).
 * level_copy_dev: level j as digest_len rows of N >> j elements (element e of node k at d_out[e * (N >> j) + k]), enqueued on
 *             `stream` behind the build.
 * verify_batch: HOST arrays, item-major: roots[t * digest_len + e], paths[((t * depth) + j) * digest_len + e], rows[t * width + e],
 *             every word reduced mod p; verdicts_out[t] = 1 if the path leads from the row to the root, else 0.  All items share
 *             depth (<= 63; 0 compares the leaf digest with the root), width and parameters; an item's whole walk runs inside one
 *             launch, one lane per state register when k <= "rescue_tree_split_max_nodes", one lane per item otherwise.  Runs on
 *             the library stream and waits.  k == 0: SC_OK, nothing is launched.
 * path_trace_dev: every state of k walks from a leaf DIGEST to the root, for trees whose node is one permutation (2 * digest_len <
 *             rate), as the execution trace a STARK proves membership with (rescue_membership.py).  HOST inputs, item-major like
 *             verify_batch's with the leaf digests in the place of the rows: leaves[t * digest_len + e], indices[t],
 *             paths[((t * depth) + j) * digest_len + e], every word reduced mod p.  DEVICE output of k * W * T elements,
 *             W = m + digest_len + 1 registers (the state, the sibling, the direction bit), T = depth * (rounds + 1) + 1 rows:
 *             register s of item t's row r at d_out[((W * t + s) * T) + r], canonical residues -- one register of one item is one
 *             run.  Row 0: the leaf digest, zeros elsewhere.  Row 1 + j * (rounds + 1): the digest reached and paths[..j..] in the
 *             order bit j of the index says (the walk's own digest first when the bit is 0), then 1, then zeros; the `rounds` rows
 *             behind it: the state after each round; all rounds + 1 rows carry paths[..j..] and the bit in registers m .. m + d.
 *             Registers 0 .. d - 1 of row T - 1 are the root the walk reaches.  One launch, one lane per state register when
 *             k <= "rescue_tree_split_max_nodes", one lane per item otherwise; the same bits.  The call only enqueues on `stream`,
 *             apart from staging its inputs: up to 8 KiB per array they travel as kernel arguments and nothing is waited for,
 *             larger ones are copied into a block of the call's own and `stream` is waited for once, BEFORE the kernel is
 *             enqueued.  No shared scratch, no one-stream rule: calls on different streams do not disturb one another.  k == 0:
 *             SC_OK, nothing is launched.
 * SC_ERR_BAD_ARG, before anything is enqueued or allocated (*tree and the outputs stay as they were): m outside 2 .. 8, rate outside
 * 2 .. m - 1, digest_len outside 1 .. rate, rounds outside 1 .. 27, width == 0, N zero or no power of two, ld < N, a NULL pointer
 * where one is needed, a constant not below p, an index not below N (open) or 1 << depth (verify, path_trace), depth > 63, a level
 * above log2 N, byte counts that wrap; path_trace also: depth == 0, 2 * digest_len >= rate. */
typedef struct sc_rescue_tree sc_rescue_tree_t;   /* device-resident Rescue-Prime Merkle tree, all levels kept */
int sc_rescue_merkle_build_dev(const void* d_rows, uint64_t ld, uint64_t width, uint64_t N, uint64_t digest_len,
                               uint64_t m, uint64_t rate, const void* params, uint64_t rounds,
                               sc_rescue_tree_t** tree, void* stream);
int sc_rescue_merkle_root(sc_rescue_tree_t* tree, void* root_out /* digest_len elements, host */);
int sc_rescue_merkle_open_batch(const sc_rescue_tree_t* tree, const uint64_t* indices, uint64_t k,
                                void* paths_out /* host: k * log2 N * digest_len elements */);
int sc_rescue_merkle_level_copy_dev(const sc_rescue_tree_t* tree, uint64_t level, void* d_out, void* stream);
int sc_rescue_merkle_verify_batch(const void* roots, const uint64_t* indices, const void* paths, const void* rows,
                                  uint64_t k, uint64_t depth, uint64_t width, uint64_t digest_len,
                                  uint64_t m, uint64_t rate, const void* params, uint64_t rounds, uint8_t* verdicts_out);
int sc_rescue_merkle_path_trace_dev(const void* leaves, const uint64_t* indices, const void* paths, uint64_t k, uint64_t depth,
                                    uint64_t digest_len, uint64_t m, uint64_t rate, const void* params, uint64_t rounds,
                                    void* d_out, void* stream);
uint64_t sc_rescue_merkle_leaves(const sc_rescue_tree_t* tree);
int sc_rescue_merkle_free(sc_rescue_tree_t* tree);

/* ---- proof-of-work grinding on the transcript (grinding.py) ------------------------------------------------------
 * pow_value(seed, nonce) = the little-endian u64 of SHAKE-256(seed (32 bytes) || nonce (8 bytes, little-endian)).digest(8): one
 * Keccak-f[1600] per trial.  A nonce is accepted at `bits` iff pow_value >> (64 - bits) == 0.
 * sc_grind:       the SMALLEST accepted nonce in [start, start + max_nonces) into *nonce_out and *found_out = 1; *found_out = 0 (and
 *                 *nonce_out untouched) when the range holds none.  The search runs on the device in windows of "grind_window" trials,
 *                 ascending, one lane per trial, and stops behind the first window with a hit (one more window may have been queued);
 *                 the result does not depend on the window.  The call returns when the answer is on the host; meanwhile other
 *                 threads may call the library (another search on another stream included).  The temporaries are the call's own: no
 *                 shared scratch, no one-stream rule.  max_nonces == 0: SC_OK, *found_out = 0.
 * sc_grind_batch: the same for `count` seeds (seeds: count * 32 bytes) over the same range, in shared launches: the members ride one
 *                 grid, a member with a hit is left out of the launches that follow, and the call ends when every member has a hit
 *                 or the range is exhausted.  nonces_out[m] is written only where found_out[m] = 1.  count == 0: SC_OK, nothing is
 *                 touched.  At most 65535 seeds.
 * sc_grind_host:  sc_grind on one host core (csrc/transcript.h's Keccak-f): the baseline of the measurement, no device needed.
 * SC_ERR_BAD_ARG, before anything is enqueued: bits outside 1 .. 63, start + max_nonces above 2^64, a NULL pointer where one is needed. */
int sc_grind(const uint8_t seed32[32], int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonce_out, int* found_out, void* stream);
int sc_grind_batch(const uint8_t* seeds, uint64_t count, int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonces_out,
                   uint8_t* found_out, void* stream);
int sc_grind_host(const uint8_t seed32[32], int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonce_out, int* found_out);

/* ---- FRI split-and-fold : code/fri.py:85 ---------------------------------------------------- */
/* out[i] = 2^-1 * ((1 + alpha/(offset*omega^i)) * in[i] + (1 - alpha/(offset*omega^i)) * in[N/2+i]), i < N/2 */
int sc_fri_fold(const void* in, uint64_t N, const uint64_t alpha[2], const uint64_t offset[2], const uint64_t omega[2], void* out);
int sc_fri_fold_dev(const void* d_in, uint64_t N, const uint64_t alpha[2], const uint64_t offset[2], const uint64_t omega[2], void* d_out, void* stream);

/* ---- Merkle : code/merkle.py:6-27 ------------------------------------------------------------ */
/* leaf = BLAKE2b-512(decimal ASCII of the residue) (algebra.py:53-57, merkle.py:14); node = H(left||right) */
int sc_merkle_commit(const void* elems, uint64_t N, uint8_t root_out[64]);                 /* Merkle.commit, merkle.py:13-14 */
int sc_merkle_build(const void* elems, uint64_t N, uint8_t root_out[64], sc_merkle_t** tree);
int sc_merkle_build_dev(const void* d_elems, uint64_t N, uint8_t root_out[64], sc_merkle_t** tree, void* stream); /* sync (returns root) */
/* The commit loop of Fri.commit (fri.py:66-94) without idle time on either side: the build is only ENQUEUED (the caller prepares
 * the next round meanwhile); sc_merkle_root waits for it (once) and returns the root -- it works on every tree.
 * sc_fri_fold_commit_dev = one round in one call: the fold of fri.py:85 into d_out (N/2 elements), then the asynchronous
 * build of the tree over d_out.  Fetch the root (or free the tree) before destroying a caller-owned stream the build ran on. */
int sc_merkle_build_async_dev(const void* d_elems, uint64_t N, sc_merkle_t** tree, void* stream);
/* the same, for a tree whose ROOT nobody is expected to read (a rank's local subtree of a sharded commit, whose sub-root level is
 * copied out with sc_merkle_level_copy_dev on the same stream): takes none of the 256 pinned root slots and runs no publish
 * kernel, so any number of such trees may be alive; sc_merkle_root still works (it then waits for the whole device). */
int sc_merkle_build_noroot_dev(const void* d_elems, uint64_t N, sc_merkle_t** tree, void* stream);
int sc_merkle_root(sc_merkle_t* tree, uint8_t root_out[64]);
int sc_fri_fold_commit_dev(const void* d_in, uint64_t N, const uint64_t alpha[2], const uint64_t offset[2], const uint64_t omega[2], void* d_out,
                           sc_merkle_t** tree, void* stream);
/* Fri.commit's whole round loop (fri.py:66-94) in one call, the Fiat-Shamir step included: per round the tree of the codeword
 * (built asynchronously, the root polled from its pinned slot), alpha = Field.sample(SHAKE-256(pickle.dumps(transcript)))
 * (ip.py:18-25, algebra.py:116-120) computed by the library, and the fold of fri.py:85 enqueued the moment alpha exists --
 * nothing crosses the language boundary between a root arriving and the next launch.  The transcript is the list of the
 * `prior_count` byte strings already in the proof stream (prior_lens[i] < 256 bytes each, concatenated in prior_data; the
 * caller checks that the stream holds nothing else) followed by this call's roots: that list has a fixed pickle layout
 * (csrc/transcript.h).  omega and offset are squared from round to round (fri.py:86-87).
 * Out: trees_out[rounds] ([0] over d_codeword), vecs_out[rounds - 1] folded codewords (library-owned: sc_vec_free),
 * roots_out[64 * rounds], alphas_out[2 * (rounds - 1)].  SC_ERR_UNSUPPORTED: the transcript does not have the fixed layout. */
int sc_fri_commit_dev(const void* d_codeword, uint64_t N, const uint64_t offset[2], const uint64_t omega[2], uint32_t rounds,
                      const void* prior_data, const uint32_t* prior_lens, uint64_t prior_count,
                      sc_vec_t** vecs_out, sc_merkle_t** trees_out, uint8_t* roots_out, uint64_t* alphas_out, void* stream);
/* Fri.prove (code/fri.py:115-130) in ONE call: the commit phase as above (fri.py:66-94), then -- without leaving the library --
 * the last codeword in the clear (fri.py:91), the challenge SHAKE-256(pickle.dumps([prior..., roots..., last codeword])) of
 * ip.py:18-25 (the FieldElement list pickled as CPython pickles it: csrc/proof_pickle.h), Fri.sample_indices (fri.py:36-51, :122;
 * BLAKE2b of seed + counter zero bytes), the positions each round opens (fri.py:98-113, :124-128) and ONE kernel that gathers every
 * opened element and authentication path of the proof.  `extra_count` further (tree, device vector) pairs of N leaves -- FastStark's
 * committed codewords, fast_stark.py:154-175 -- are opened in the same launch at the sorted positions
 * {i, i + extra_shift, i + N/2, i + extra_shift + N/2 (mod N)} over the top-level indices i (written to extra_indices_out, 4 *
 * num_tests of them).  Openings per pair, in this order: codeword j of the commit phase: [a (num_tests), b = a + half (num_tests)] if
 * j < rounds - 1 -- the c positions of the round before (= that round's a) are this codeword's a or b, whichever half they lie in, and
 * are opened once --, the last codeword [c (num_tests)]; every further pair: the sorted positions.
 * `answers` (answers_bytes >= the sum below) = [opened elements, 16 bytes each, padded to a multiple of 256 bytes][paths, 64 * log2
 * N_pair bytes per opening][the positions, u64 each], pairs concatenated.  A buffer of sc_host_alloc is written by the kernel itself
 * across the bus (no staging copy); any other host pointer works through two copies.  Outputs of the commit phase as for
 * sc_fri_commit_dev -- or vecs_out = trees_out = NULL (alphas_out may be NULL as well): nothing reads the folded codewords and
 * their trees once the openings are on the host, and the library then hands their memory back before it returns;
 * last_codeword_out: 16 * (N >> (rounds - 1)) bytes; top_indices_out: num_tests.
 * SC_ERR_UNSUPPORTED: a transcript or shape this entry does not serve (the caller runs the phases one by one). */
int sc_fri_prove_dev(const void* d_codeword, uint64_t N, const uint64_t offset[2], const uint64_t omega[2], uint32_t rounds, uint32_t num_tests,
                     const void* prior_data, const uint32_t* prior_lens, uint64_t prior_count,
                     uint64_t extra_count, const sc_merkle_t* const* extra_trees, const void* const* extra_vecs, uint64_t extra_shift,
                     sc_vec_t** vecs_out, sc_merkle_t** trees_out, uint8_t* roots_out, uint64_t* alphas_out,
                     void* last_codeword_out, uint64_t* top_indices_out, uint64_t* extra_indices_out,
                     void* answers, uint64_t answers_bytes, void* stream);
/* sc_fri_prove_dev for a Fri with grinding (Fri(..., grinding_bits), grinding.py): the same arguments, then grinding_bits (0 .. 63;
 * 0 = sc_fri_prove_dev exactly) and nonce_out.  Between the seed over the transcript with the last codeword and the sampling of the
 * indices the call finds the smallest nonce accepted at grinding_bits with that seed (sc_grind's search, on `stream`), writes it to
 * *nonce_out, appends it to the transcript as the plain integer the prover pushes, and samples the indices from the hash of that
 * transcript.  The caller pushes the nonce between the last codeword and the query phase's objects. */
int sc_fri_prove_grind_dev(const void* d_codeword, uint64_t N, const uint64_t offset[2], const uint64_t omega[2], uint32_t rounds, uint32_t num_tests,
                           const void* prior_data, const uint32_t* prior_lens, uint64_t prior_count,
                           uint64_t extra_count, const sc_merkle_t* const* extra_trees, const void* const* extra_vecs, uint64_t extra_shift,
                           sc_vec_t** vecs_out, sc_merkle_t** trees_out, uint8_t* roots_out, uint64_t* alphas_out,
                           void* last_codeword_out, uint64_t* top_indices_out, uint64_t* extra_indices_out,
                           void* answers, uint64_t answers_bytes, void* stream, int grinding_bits, uint64_t* nonce_out);
/* pinned, device-visible host memory from a pool kept by the library (an allocation of megabytes costs hundreds of microseconds):
 * what sc_fri_prove_dev's query kernel writes a proof's openings to */
/* diagnostics of the persistent tail kernel of the commit phase (csrc/fri_tail.cuh): out[0] = launches so far, out[1] = launches
 * whose wait for a challenge or a peer workgroup gave up, after which the rounds were finished with the per-round launches */
int sc_fri_tail_stats(uint64_t out[2]);
int sc_host_alloc(uint64_t bytes, void** out);
int sc_host_free(void* p);
/* the host-side pieces of that step on their own (no GPU needed; tests pin them to hashlib / pickle):
 * SHAKE-256 (FIPS 202); Field.sample = big-endian integer of the bytes mod p; pickle.dumps of a list of `count` byte strings
 * (*out_len = bytes needed, copied into out when out_cap suffices) */
int sc_shake256(const void* in, uint64_t len, void* out, uint64_t out_len);
/* ProofStream.serialize() (code/ip.py:18-19: pickle.dumps(self.objects), protocol 4) of a proof stream given as a DESCRIPTION of
 * its object graph instead of Python objects -- lists, bytes, authentication paths, triples, FieldElements with their object
 * identities (format: csrc/proof_pickle.h).  Byte-identical to CPython's pickler.  moduli: nfields little-endian moduli of
 * modulus_bytes each.  *out_len = bytes needed; copied into out when out_cap suffices.  Host only (no GPU needed). */
int sc_pickle_proof(const void* ops, uint64_t ops_len, const void* moduli, uint32_t nfields, uint32_t modulus_bytes, void* out, uint64_t out_cap, uint64_t* out_len);
/* Field.sample (algebra.py:116-120) of `count` host byte strings of `width` <= 32 bytes each, straight into device memory: the
 * randomizer polynomial of FastStark.prove (fast_stark.py:117: one os.urandom(17) draw per coefficient) without a Python object
 * per coefficient.  Synchronous (the bytes are the caller's host memory). */
int sc_sample_bytes_dev(const void* bytes, uint64_t count, uint32_t width, void* d_out, void* stream);
/* The randomized trace matrix of a batch of proofs (fast_stark.py:79-81 for every member in one launch): column c = m * registers
 * + s of d_out (at element c * ld_out) is the trace column at element c * ld_trace of d_trace (`rows` elements) followed by `extra`
 * randomizer values; element rows + r is Field.sample of the `width` (1..32) bytes at draws + m * draws_stride + (r * registers + s)
 * * width -- the reference's draw order, row by row, register by register.  `draws` is HOST memory, draws_stride the bytes from one
 * member's block to the next (at least extra * registers * width when members > 1).  rows == 0 (d_trace may be NULL) with
 * registers == 1 samples one polynomial of `extra` coefficients per member.  ld_out >= rows + extra, ld_trace >= rows; the output
 * may not overlap the trace.  members == 0, registers == 0 or rows + extra == 0: nothing happens.  Synchronous when there are
 * draws (the bytes are the caller's host memory), else enqueued on `stream`. */
int sc_randomized_columns_dev(const void* d_trace, uint64_t rows, uint64_t ld_trace, uint64_t members, uint64_t registers, const void* draws, uint64_t draws_stride,
                              uint64_t extra, uint32_t width, void* d_out, uint64_t ld_out, void* stream);
/* The same with the draws made by the library: `count` times getrandom(width bytes) -- what os.urandom(width) is -- split over
 * host threads into a pinned staging buffer, one asynchronous copy, Field.sample on the device.  Enqueued on `stream`.  For
 * callers whose os.urandom is the operating system's (a patched, seeded os.urandom must go through sc_sample_bytes_dev, whose
 * bytes and order are the caller's). */
int sc_sample_urandom_dev(uint64_t count, uint32_t width, void* d_out, void* stream);
/* start those draws NOW on host threads and return: a later sc_sample_urandom_dev of the same (count, width) uses them (the prover
 * calls this at the top of a proof; the kernel randomness is drawn while the GPU works on the trace) */
int sc_urandom_prefetch(uint64_t count, uint32_t width);
int sc_field_sample(const void* bytes, uint64_t len, uint64_t out[2]);
/* ... and of sc_fri_prove_dev's index sampling: BLAKE2b-512 (RFC 7693, unkeyed) of a message of any length; Fri.sample_indices
 * (fri.py:36-51) for a power-of-two `size`: `number` indices below size, pairwise distinct modulo reduced_size, candidate k = the
 * big-endian integer of blake2b(seed + k zero bytes) mod size (SC_ERR_UNSUPPORTED where the reference's assertion fails) */
int sc_blake2b(const void* in, uint64_t len, uint8_t out[64]);
/* SHAKE-256(pickle.dumps(items + [root])) (ip.py:18-25) in the split form the commit loops use: every whole rate block in front of
 * the pending 64-byte root absorbed before the root is known, the rest after (csrc/transcript.h: PendingChallenge) */
int sc_transcript_challenge(const void* data, const uint32_t* lens, uint64_t count, const uint8_t root[64], uint8_t* out, uint64_t out_len);
int sc_fri_sample_indices(const void* seed, uint64_t seed_len, uint64_t size, uint64_t reduced_size, uint32_t number, uint64_t* out);
int sc_transcript_bytes(const void* data, const uint32_t* lens, uint64_t count, void* out, uint64_t out_cap, uint64_t* out_len);
int sc_merkle_open(const sc_merkle_t* tree, uint64_t index, uint8_t* path_out /* 64*log2 N */); /* Merkle.open, merkle.py:16-27 */
int sc_merkle_open_batch(const sc_merkle_t* tree, const uint64_t* indices, uint64_t k, uint8_t* paths_out /* k*64*log2 N */);
/* The batched verifier's checks (FastStark.verify_batch, Fri.verify_batch; rows as in csrc/merkle_verify.cuh), synchronous, host buffers
 * in and out, any row count: the rows go to the device in chunks through one bounded pinned staging buffer ("verify_stage_kb").
 * sc_merkle_verify_batch: n rows of 48 bytes {u64 position, u64 path, u32 root, u32 depth <= 64, u32 kind, u32 0, u64 leaf[2]} --
 * Merkle.verify_(roots[root], position, digests[path .. path + depth - 1], leaf) with the leaf the BLAKE2b-512 of the decimal ASCII of
 * the 128-bit residue leaf[0] + 2^64 leaf[1] (kind 0) or digests[leaf[0]] (kind 1); digests and roots 64 bytes each.  verdicts_out[i]
 * = 1 when the path leads to the root, else 0 (also when position >= 2^depth).  Each row is staged with its own path and, for kind 1,
 * its leaf digest on its own, so a leaf digest may lie anywhere in `digests`; rows whose paths follow each other in `digests` go to
 * the device in the fewest chunks.
 * sc_fri_colinearity_batch: n rows of 80 bytes {u64 a, u64 b, u32 round, u32 0[3], y_a, y_b, y_c} over rounds of 48 bytes {offset,
 * omega, alpha}, all residues 16 bytes little-endian -- test_colinearity([(x_a, y_a), (x_b, y_b), (alpha, y_c)]) with x = offset *
 * omega^e: verdicts_out[i] = 1 / 0, or 2 (undecided: two abscissas coincide or an input is not below p; the caller decides).
 * A row that indexes outside the digests, roots or rounds given: SC_ERR_BAD_ARG, nothing is run. */
int sc_merkle_verify_batch(const void* rows, uint64_t n, const void* digests, uint64_t n_digests, const void* roots, uint64_t n_roots, uint8_t* verdicts_out);
int sc_fri_colinearity_batch(const void* rows, uint64_t n, const void* rounds, uint64_t n_rounds, uint8_t* verdicts_out);
/* The verifier's third check as rows (csrc/combination.cuh): the nonlinear combination recomputed at the opened points
 * (fast_stark.py:236-284), for one AIR on one FRI domain and any number of proofs (members).  Synchronous, host buffers in and out, any
 * row count: the rows go to the device in chunks through the same staging buffer ("verify_stage_kb"); a chunk is three launches -- the
 * point matrix, the AIR under the plan of sc_mpoly_eval_columns_dev, the weighted sum -- and one wait.  All residues are 16 bytes
 * little-endian.  The AIR's variables are X, `registers` current and `registers` next values: nvars = 1 + 2 registers <= 255; ncons /
 * nterms / exps / coefs as sc_mpoly_eval_columns_dev takes them (exps: [terms][nvars] bytes, so no term can name a variable beyond
 * nvars).  Per member: 1 + 2 ncons + 2 registers weights (randomizer; per transition quotient plain and shifted; per boundary quotient
 * plain and shifted), and polys[(m * registers + s) * 4 ..] = {offset, length} of register s's boundary zerofier, then of its boundary
 * interpolant, in elements of `pool`, lowest degree first; length 0 is the zero polynomial.
 * A row is 64 + 32 registers bytes: {u64 member, u64 index, claimed, randomizer leaf, transition-zerofier leaf, registers boundary-quotient
 * leaves at `index`, registers at successor = (index + step) mod domain_length}.  With x = generator * omega^index (x' at the successor),
 * trace_s = quotient_s * zerofier_s(x) + interpolant_s(x), point = (x, trace at x, trace at x'):
 *   total = randomizer * w_0 + sum_c (AIR_c(point) / zerofier leaf) * (w + x^transition_shifts[c] * w') + sum_s quotient_s * (w + x^boundary_shifts[s] * w')
 * verdicts_out[i] = 1 when total == claimed, else 0; 2 (undecided: the caller decides) when the zerofier leaf is 0 or a residue the row
 * uses -- its own, its member's weights or coefficient lists, generator, omega -- is not below p.
 * n == 0: SC_OK.  SC_ERR_BAD_ARG, nothing run and nothing written: a null pointer, registers 0 or above 127, domain_length no power of
 * two, step 0, a row with index >= domain_length or member >= members, a coefficient list outside the pool, a coefficient of the AIR
 * not below p. */
typedef struct sc_combination {
    uint64_t registers, ncons;
    const uint64_t* nterms;             /* [ncons] */
    const uint8_t* exps;
    const void* coefs;
    uint64_t generator[2], omega[2];
    uint64_t domain_length, step;
    const uint64_t* transition_shifts;  /* [ncons] */
    const uint64_t* boundary_shifts;    /* [registers] */
    uint64_t members;
    const void* weights;                /* [members][1 + 2 ncons + 2 registers] */
    const uint64_t* polys;              /* [members][registers][4] */
    const void* pool;
    uint64_t pool_len;                  /* elements */
} sc_combination_t;
int sc_stark_combination_batch(const sc_combination_t* shared, const void* rows, uint64_t n, uint8_t* verdicts_out);
/* opened elements AND their paths in one call: elems_out[i] = d_elems[indices[i]] (d_elems = the device vector the tree was built from) */
int sc_merkle_query_dev(const sc_merkle_t* tree, const void* d_elems, const uint64_t* indices, uint64_t k, void* elems_out, uint8_t* paths_out);
/* several (tree, vector) pairs in one round trip (the query phase of Fri.prove, fri.py:124-128): counts[t] of the concatenated
 * `indices` belong to pair t; outputs concatenated in the same order (16 bytes per element, 64 * log2 N_t bytes per path) */
int sc_merkle_query_multi_dev(uint64_t n, const sc_merkle_t* const* trees, const void* const* d_elems, const uint64_t* indices, const uint64_t* counts,
                              void* elems_out, uint8_t* paths_out);
/* pieces for a tree sharded over ranks: copy of one level of a built tree (level 0 = leaf digests; (N >> level) * 64 bytes),
 * a tree whose level 0 is given digests, and the fold of fri.py:85 on a rank's column slab [rows][cols] of the codeword
 * viewed as a rows x R matrix (index i = row*R + col_base + col; the partner i + N/2 is row + rows/2 of the same slab) */
int sc_merkle_level_copy_dev(const sc_merkle_t* tree, int level, void* d_out, void* stream);
int sc_merkle_from_digests_dev(const void* d_digests, uint64_t count, uint8_t root_out[64], sc_merkle_t** tree, void* stream); /* root_out NULL: only enqueued, sc_merkle_root waits */
int sc_fri_fold_slab_dev(const void* d_in, uint64_t rows, uint64_t cols, uint64_t R, uint64_t col_base, const uint64_t alpha[2], const uint64_t offset[2],
                         const uint64_t omega[2], void* d_out, void* stream);
/* that fold AND the local Merkle subtree over the folded slab in one call (a round of the sharded Fri.commit, fri.py:73-88, on one
 * rank): from 256 folded elements up the tree's leaf stage computes the fold itself; the tree is a *_noroot_dev tree (only
 * enqueued; its sub-root level is read with sc_merkle_level_copy_dev on the same stream) */
int sc_fri_fold_slab_build_dev(const void* d_in, uint64_t rows, uint64_t cols, uint64_t R, uint64_t col_base, const uint64_t alpha[2], const uint64_t offset[2],
                               const uint64_t omega[2], void* d_out, sc_merkle_t** tree, void* stream);
uint64_t sc_merkle_leaves(const sc_merkle_t* tree);
int sc_merkle_free(sc_merkle_t* tree);

/* ---- Row commitments: ONE tree over the rows of a matrix of codewords (not in the reference) ------------------- */
/* leaf i = BLAKE2b-512(col[0][i] || ... || col[w-1][i], person = "sc-merkle-row"), 16 little-endian bytes per value, digest 64, no
 * key; node = H(left || right) as above.  The personalisation keeps leaves and nodes apart (a row of 8 values is 128 bytes, a node's
 * message).  The values are hashed as they lie in memory: nothing is reduced.  d_cols: a HOST array of w device pointers, each to N
 * elements (N a power of two; the columns need not be neighbours); the result is an ordinary sc_merkle_t: sc_merkle_root,
 * sc_merkle_open_batch, sc_merkle_level_copy_dev and sc_merkle_free work on it unchanged.  N == 1: the root is the leaf digest and
 * paths are empty.  One lane per row, ceil(16 w / 128) compressions per leaf (csrc/merkle_rows.cuh); from 256 leaves up the leaf stage
 * is the entry of the fused subtree launch of the decimal trees.
 * build_dev:       synchronous, the root to root_out (may be NULL when `tree` is given; `tree` may be NULL when root_out is given).
 * build_async_dev: only enqueues; sc_merkle_root waits.  Fetch the root (or free the tree) before destroying a caller-owned stream.
 *                  Both builds take the caller's stream; the pointer table travels as a kernel argument and the tree is the call's
 *                  own allocation: no shared scratch, no one-stream rule -- the columns must be complete on `stream`, and builds on
 *                  different streams do not disturb one another.
 * query_dev:       for k positions, the w values of each row (rows_out: [k][w], 16 bytes each) and its path (paths_out: 64 * log2 N
 *                  bytes per position) in ONE launch on the library stream; synchronous.  d_cols, w: the columns the tree was built
 *                  from, whose build must be complete or ordered before the library stream (sc_merkle_root has returned).  Outputs
 *                  inside a buffer of sc_host_alloc are written by the kernel itself; other host memory is served through the shared
 *                  staging scratch, so queries keep the one-stream rule like sc_merkle_query_dev.  k == 0: SC_OK.
 * row_leaf:        host only, no GPU: the leaf digest of one row of w values (16 bytes each) -- the specification, for tests and callers
 *                  without Python.
 * SC_ERR_BAD_ARG, with nothing enqueued and nothing written: w == 0, w > SC_MERKLE_ROWS_MAX_COLUMNS, a NULL column or table, an index
 * >= N, a NULL output that is needed; SC_ERR_NOT_POW2: N no power of two. */
#define SC_MERKLE_ROWS_MAX_COLUMNS 256
int sc_merkle_rows_build_dev(const void* const* d_cols, uint64_t w, uint64_t N, uint8_t root_out[64], sc_merkle_t** tree, void* stream);
int sc_merkle_rows_build_async_dev(const void* const* d_cols, uint64_t w, uint64_t N, sc_merkle_t** tree, void* stream);
int sc_merkle_rows_query_dev(const sc_merkle_t* tree, const void* const* d_cols, uint64_t w, const uint64_t* indices, uint64_t k, void* rows_out, uint8_t* paths_out);
int sc_merkle_row_leaf(const void* row, uint64_t w, uint8_t out[64]);   /* host only */

/* ---- pair leaves for FRI (not in the reference; Fri(pair_leaves=True)) ------------------------------------------------ */
/* A round's codeword cw of n >= 2 elements is committed as the row tree of its two halves: n/2 leaves, leaf i = the row leaf of
 * (cw[i], cw[i + n/2]) -- sc_merkle_rows_build*_dev on the two pointers {cw, cw + n/2} builds it, and the tree is an ordinary sc_merkle_t.
 * fold_pairs_commit_dev: the pair twin of sc_fri_fold_commit_dev, one round of the commit phase in one call, enqueue only: the fold of
 *             fri.py:85 of d_in (N elements, N a power of two >= 4) into d_out (N/2 elements, bit for bit what sc_fri_fold_dev writes)
 *             and the asynchronous build of the pair tree over d_out (N/4 leaves).  From 256 leaves up the leaf stage of the tree
 *             computes the fold itself: a lane folds both members of its pair, stores them and hashes them out of registers.  No shared
 *             scratch: free of the one-stream rule, like sc_fri_fold_commit_dev.  sc_merkle_root waits for the root.
 * pairs_query_dev: every opening of a proof's query phase in ONE launch on the library stream; synchronous.  Codeword j: 2 L_j elements
 *             at d_codewords[j] under the pair tree trees[j] of L_j leaves; counts[j] of the concatenated `indices` belong to it.  Opening
 *             i of codeword j writes the pair {cw[a], cw[a + L_j]} (32 bytes) to pairs_out and the 64 * log2 L_j bytes of leaf a's path to
 *             paths_out, both packed codeword after codeword in the order of `indices`.  A tree that was only enqueued is waited for.
 *             Outputs inside a buffer of sc_host_alloc are written by the kernel itself; other host memory is served through the shared
 *             staging scratch (the one-stream rule of sc_merkle_query_multi_dev).  n == 0 or all counts 0: SC_OK.
 * SC_ERR_BAD_ARG, with nothing enqueued and nothing written: a NULL handle, codeword, table or needed output, an index >= L_j;
 * SC_ERR_NOT_POW2: N no power of two, or below 4. */
int sc_fri_fold_pairs_commit_dev(const void* d_in, uint64_t N, const uint64_t alpha[2], const uint64_t offset[2], const uint64_t omega[2], void* d_out,
                                 sc_merkle_t** tree, void* stream);
int sc_fri_pairs_query_dev(uint64_t n, const sc_merkle_t* const* trees, const void* const* d_codewords, const uint64_t* indices, const uint64_t* counts,
                           void* pairs_out, uint8_t* paths_out);
/* Fri.prove with pair leaves in ONE call: the arguments of sc_fri_prove_grind_dev (grinding_bits = 0: no proof of work, nonce_out may be
 * NULL), the same steps, over pair trees.
 * Commit phase: codeword r (n_r = N >> r elements) under the row tree of {cw, cw + n_r/2} (n_r/2 leaves); round 0's tree is started
 *             asynchronously, the rounds whose output has more than 2^16 elements use the launches of sc_fri_fold_pairs_commit_dev, each root
 *             is polled from its pinned slot and the challenge computed in the library as in sc_fri_commit_dev; from 2^16 elements down the
 *             rounds run in the pair form of the persistent tail kernel (csrc/fri_tail.cuh: a lane folds both members of a pair and hashes
 *             the 32-byte row leaf out of registers), with the per-round launches as the fall-back when the kernel is switched off
 *             (sc_set_tuning("fri_tail", 0), STARKCORE_FRI_TAIL=0), not taken or gave up (counted in sc_fri_tail_stats).
 * Between commit and query: as in sc_fri_prove_dev -- the last codeword in the clear, the challenge over [prior..., roots..., last
 *             codeword], the proof of work (grinding_bits > 0), Fri.sample_indices.
 * Openings:   one launch.  Codeword j < rounds - 1: the num_tests pairs {cw_j[a], cw_j[a + n_j/2]} and the paths of leaf a = index mod
 *             n_j/2 over the top-level indices; nothing of the last codeword.  The `extra_count` further (ordinary tree, device vector)
 *             pairs: as in sc_fri_prove_dev, at the four-fold sorted positions written to extra_indices_out.
 * `answers`:  four sections, each contiguous and starting at a multiple of 256 bytes, each codeword after codeword:
 *               [pairs            32 bytes per opening: num_tests per codeword j < rounds - 1]
 *               [extra elements   16 bytes per opening: 4 num_tests per further pair]
 *               [paths            64 * log2(n_j/2) bytes per pair opening, then 64 * log2 N per opening of a further pair]
 *               [positions        u64: the leaf numbers a (num_tests per codeword), then the sorted positions of each further pair]
 *             answers_bytes >= the four section lengths, the first three rounded up to multiples of 256.  A buffer of sc_host_alloc is
 *             written by the kernel itself; any other host pointer is served through the staging copy.
 * Outputs:    as sc_fri_prove_dev's.  With vecs_out = trees_out = NULL the folded codewords and their trees go back to the pools before the
 *             call returns; given, trees_out[r] is an ordinary sc_merkle_t of n_r/2 leaves (sc_fri_pairs_query_dev, sc_merkle_open_batch).
 * Refused with nothing enqueued and nothing written -- SC_ERR_NOT_POW2: N no power of two, or N >> (rounds - 1) < 2; SC_ERR_BAD_ARG: a NULL
 * that is needed, num_tests == 0 or > N >> (rounds - 1), rounds < 2, answers_bytes too small, grinding_bits outside 0 .. 63;
 * SC_ERR_UNSUPPORTED: a transcript outside the fixed layout, or rounds + extra_count > 32 (the caller runs the phases one by one). */
int sc_fri_prove_pairs_dev(const void* d_codeword, uint64_t N, const uint64_t offset[2], const uint64_t omega[2], uint32_t rounds, uint32_t num_tests,
                           const void* prior_data, const uint32_t* prior_lens, uint64_t prior_count,
                           uint64_t extra_count, const sc_merkle_t* const* extra_trees, const void* const* extra_vecs, uint64_t extra_shift,
                           sc_vec_t** vecs_out, sc_merkle_t** trees_out, uint8_t* roots_out, uint64_t* alphas_out,
                           void* last_codeword_out, uint64_t* top_indices_out, uint64_t* extra_indices_out,
                           void* answers, uint64_t answers_bytes, void* stream, int grinding_bits, uint64_t* nonce_out);

/* ---- Merkle forests: Merkle.commit (merkle.py:13-14) of `count` arrays of N leaves each in one set of launches ------------------ */
/* d_elems: a device matrix [count][N] of residues, row t = the leaves of tree t; N a power of two >= 2, count >= 1.  All levels of all
 * trees are kept (tree-major, csrc/merkle_forest.cuh).  The largest forest an entry takes has SC_FOREST_MAX_LEAVES leaves in total
 * (count * N; the fold: of its input): above it SC_ERR_UNSUPPORTED and the caller splits the batch.  N not a power of two or below 2,
 * count 0, a NULL argument: SC_ERR_BAD_ARG.  Nothing is enqueued by a call that fails.  Enqueue only: sc_merkle_forest_roots waits.
 * The roots travel to pinned memory of the forest's own (the pool of sc_host_alloc), written by the launch that computes them: a
 * forest takes none of the 256 pinned slots the asynchronous single trees and the deferred checks share. */
#define SC_FOREST_MAX_LEAVES (1ull << 24)
int sc_merkle_forest_build_dev(const void* d_elems, uint64_t N, uint64_t count, sc_merkle_forest_t** forest, void* stream);
/* One round of Fri.commit (fri.py:73-88) for `count` codewords at once: row t of d_out [count][N/2] = the split-and-fold (fri.py:85) of
 * row t of d_in [count][N] with its own challenge alphas_host[2t .. 2t+1] (packed canonical residues in HOST memory: they come from the
 * host's Fiat-Shamir step; offset and omega are shared), and the forest over d_out, whose leaf stage computes the fold.  Equal to
 * sc_fri_fold_dev row by row, bit for bit.  N = 2 leaves trees of one leaf.  Enqueue only. */
int sc_fri_fold_forest_dev(const void* d_in, uint64_t N, uint64_t count, const uint64_t* alphas_host, const uint64_t offset[2], const uint64_t omega[2], void* d_out,
                           sc_merkle_forest_t** forest, void* stream);
/* waits for the build, once, with the library's lock released: a forest has ONE owner -- no other thread may free the handle while a
 * call on it is in progress (as for every handle of this header) */
int sc_merkle_forest_roots(sc_merkle_forest_t* forest, uint8_t* roots_out /* 64 * count */);
uint64_t sc_merkle_forest_trees(const sc_merkle_forest_t* forest);
uint64_t sc_merkle_forest_leaves(const sc_merkle_forest_t* forest);                            /* per tree */
int sc_merkle_forest_free(sc_merkle_forest_t* forest);
/* sc_merkle_query_multi_dev for forests: opening i of pair p is element and path (Merkle.open, merkle.py:16-27) of leaf indices[i] of
 * tree trees[i] of forests[p] over the matrix d_elems[p]; counts[p] openings belong to pair p, concatenated; outputs concatenated in
 * the same order (16 bytes per element, 64 * log2 N_p bytes per path).  One launch for all pairs.  elems_out / paths_out inside
 * buffers of sc_host_alloc are written by the kernel itself; other host pointers are served through a copy.  A tree >= count or an
 * index >= N: SC_ERR_BAD_ARG, nothing enqueued.  Synchronous. */
int sc_merkle_forest_query_dev(uint64_t n_pairs, const sc_merkle_forest_t* const* forests, const void* const* d_elems, const uint64_t* trees, const uint64_t* indices,
                               const uint64_t* counts, void* elems_out, uint8_t* paths_out);
int sc_merkle_forest_stats(uint64_t out[2]);   /* forests built and trees in them since sc_init */

/* ---- Row forests: `count` row commitments (above) of N rows and w columns each in one set of launches ---------- */
/* Tree t is the row tree of its own w columns: leaf i = the personalised row hash of sc_merkle_rows_build_dev over tree t's values at
 * row i, nodes as everywhere; root t = the root sc_merkle_rows_build_dev gives for those columns.  In a batch the columns are not
 * count * w allocations but the columns of a few matrices, so they are described by n_segs (1 .. SC_ROW_FOREST_MAX_SEGMENTS)
 * SEGMENTS, a HOST array that travels as a kernel argument: segment s is a device matrix of count * per_tree columns, consecutive
 * columns `pitch` elements (>= N) apart, and tree t's columns are, segment after segment, columns t * per_tree .. t * per_tree +
 * per_tree - 1 of that segment.  Column c of tree t at row i lies at base_s + 16 * ((t * per_tree_s + (c - first_s)) * pitch_s + i),
 * first_s = the columns of the segments in front; w = the sum of per_tree, 1 .. SC_MERKLE_ROWS_MAX_COLUMNS.  (The batched prover:
 * the boundary-quotient codewords [K R][N] with per_tree R, then the randomizer codewords [K][N] with per_tree 1.)  The values are
 * hashed as they lie in memory.
 * build_dev:  only enqueues, on the caller's stream.  The result is an ordinary sc_merkle_forest_t (tree-major, all levels kept):
 *             sc_merkle_forest_roots / _trees / _leaves / _free / _stats work on it unchanged, and "forest_four_lane_wgs" applies as to
 *             every forest.  No shared scratch, the table is a kernel argument and the forest the call's own allocation: the build
 *             is free of the one-stream rule -- the segments must be complete on `stream`, and builds on different streams do not
 *             disturb one another.  One lane per row; level 0 is the entry of the forest's first launch (csrc/merkle_forest.cuh).
 * query_dev:  for k positions (trees[q], indices[q]), the w values of each row (rows_out: [k][w], 16 bytes each) and its path
 *             (paths_out: 64 * log2 N bytes per position) in ONE launch on the library stream; synchronous.  segs, n_segs: what the
 *             forest was built from; a build on another stream is ordered in front of the launch on the device.  Outputs inside a
 *             buffer of sc_host_alloc are written by the kernel itself; other host memory is served through the shared staging
 *             scratch, so queries keep the one-stream rule like sc_merkle_rows_query_dev.  k == 0: SC_OK.
 * A refused call enqueues nothing, writes nothing and leaves sc_merkle_forest_stats unchanged.  SC_ERR_BAD_ARG: a NULL table, handle
 * or needed output, n_segs 0 or > SC_ROW_FOREST_MAX_SEGMENTS, a NULL base, per_tree 0, w > SC_MERKLE_ROWS_MAX_COLUMNS, pitch < N,
 * N < 2, count 0, a tree >= count, an index >= N; SC_ERR_NOT_POW2: N no power of two (as the row tree); SC_ERR_UNSUPPORTED:
 * count * N > SC_FOREST_MAX_LEAVES (split the batch). */
#define SC_ROW_FOREST_MAX_SEGMENTS 8
typedef struct { const void* base; uint64_t per_tree; uint64_t pitch; } sc_row_segment_t;   /* pitch: elements between consecutive columns, >= N */
int sc_merkle_row_forest_build_dev(const sc_row_segment_t* segs, uint64_t n_segs, uint64_t N, uint64_t count, sc_merkle_forest_t** forest, void* stream);
int sc_merkle_row_forest_query_dev(const sc_merkle_forest_t* forest, const sc_row_segment_t* segs, uint64_t n_segs, const uint64_t* trees, const uint64_t* indices,
                                   uint64_t k, void* rows_out, uint8_t* paths_out);

#ifdef __cplusplus
}
#endif
#endif
