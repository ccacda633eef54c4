/*
 * ststhip.h -- C ABI of the MI355X StencilUpdate backend (libststhip.so).
 *
 * Two layers, both `extern "C"`, plain pointers and sizes, int status codes
 * (0 = success, otherwise a ststhip_status; ststhip_last_error() describes the
 * last failure of the calling thread), no exceptions across the boundary.
 *
 * Layer 0 -- runtime services underneath the C++ templates.  In the reference
 * these are the implicit services of the SYCL runtime behind
 * cuda::StencilUpdate / cuda::Grid (queue creation and wait
 * StencilStream/cuda/StencilUpdate.hpp:124-135, buffer allocation :204-205 and
 * cuda/internal/Helpers.hpp:37-45, implicit host<->device copies behind
 * host_accessor cuda/Grid.hpp:145-153, event profiling :184-198).
 *
 * Layer 1 -- the generation sweep itself for the precompiled transition
 * functions (the five example applications and the reference's self-checking
 * test function).  One call of ststhip_app_sweep() replaces the body of
 * cuda::StencilUpdate::run_simulation's loop (StencilStream/cuda/
 * StencilUpdate.hpp:212-273 AoS, :324-405 SoA) for `n_generations`
 * generations at once (temporal blocking); ststhip_app_run() replaces
 * cuda::StencilUpdate::operator() (:123-144).  This is the surface a foreign
 * language binds (ctypes stub in INTEGRATION.md; stencilstream_amd/capi.py).
 *
 * Transition functions that only exist as C++ templates in the user's
 * translation unit are compiled there (StencilStream/hip/StencilUpdate.hpp)
 * and use layer 0 only.
 */
#ifndef STSTHIP_H
#define STSTHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STSTHIP_ABI_VERSION 6

typedef enum {
    STSTHIP_OK = 0,
    STSTHIP_ERR_HIP = 1,          /* a HIP runtime call failed               */
    STSTHIP_ERR_INVALID = 2,      /* bad argument                            */
    STSTHIP_ERR_UNKNOWN_APP = 3,  /* no such precompiled transition function */
    STSTHIP_ERR_NO_DEVICE = 4,    /* no usable GPU                           */
    STSTHIP_ERR_COMM = 5          /* RCCL failure                            */
} ststhip_status;

typedef void *ststhip_stream; /* a hipStream_t; NULL = the runtime's own stream */
typedef void *ststhip_event;  /* a hipEvent_t */

/* ------------------------------------------------------------- layer 0 */
int ststhip_abi_version(void);
const char *ststhip_last_error(void);
/* Lets code on the caller's side of a callback (ststhip_sweep_fn) report why it failed. */
void ststhip_set_last_error(const char *message);

/* Select a GPU for the calling process (device < 0: keep the current HIP device) and create the
 * runtime's stream.  Idempotent.  Fails with STSTHIP_ERR_NO_DEVICE when no GPU is visible. */
int ststhip_init(int device);
int ststhip_shutdown(void);
int ststhip_device_count(int *count);
int ststhip_device_name(char *buf, size_t buf_size);
int ststhip_compute_units(int *count);

/* Device memory from a size-bucketed pool (freed blocks are reused, not returned to HIP).
 * Releases are stream-ordered: ststhip_free_async(ptr, stream) may be called while work that uses the
 * block is still queued on `stream`; the block is handed out again to the same stream at once, to any
 * other stream after a wait on the release event, and to ststhip_malloc (host order) once that event has
 * completed.  ststhip_free(ptr) = ststhip_free_async(ptr, NULL): release ordered after the runtime's own
 * stream.  A block that other streams still use must be released on a stream that was joined with them. */
int ststhip_malloc(void **ptr, size_t bytes);
int ststhip_free(void *ptr);
int ststhip_malloc_async(void **ptr, size_t bytes, ststhip_stream stream);
int ststhip_free_async(void *ptr, ststhip_stream stream);
int ststhip_pool_trim(void);
/* Pinned host memory for grids' host mirrors.  Freed blocks are kept for reuse (pinning is slow) up
 * to STSTHIP_HOST_CACHE_MIB (default 4096) MiB; ststhip_pool_trim releases them. */
int ststhip_host_malloc(void **ptr, size_t bytes);
int ststhip_host_free(void *ptr);

/* Asynchronous on `stream`; the host buffer must stay alive until the stream is synchronised. */
int ststhip_memcpy_h2d(void *dst, const void *src, size_t bytes, ststhip_stream stream);
int ststhip_memcpy_d2h(void *dst, const void *src, size_t bytes, ststhip_stream stream);
int ststhip_memcpy_d2d(void *dst, const void *src, size_t bytes, ststhip_stream stream);
int ststhip_memset(void *dst, int value, size_t bytes, ststhip_stream stream);

int ststhip_default_stream(ststhip_stream *stream);
int ststhip_stream_create(ststhip_stream *stream);
int ststhip_stream_destroy(ststhip_stream stream);
int ststhip_stream_synchronize(ststhip_stream stream);
int ststhip_stream_wait_event(ststhip_stream stream, ststhip_event event);

int ststhip_event_create(ststhip_event *event);
int ststhip_event_destroy(ststhip_event event);
int ststhip_event_record(ststhip_event event, ststhip_stream stream);
int ststhip_event_synchronize(ststhip_event event);
int ststhip_event_elapsed_ms(ststhip_event start, ststhip_event stop, float *ms);

/* Launch a kernel that lives in the caller's code object (`function` = host-side kernel symbol).
 * Used by the C++ templates so that launches share the runtime's error handling and stream. */
int ststhip_launch(const void *function, unsigned grid_x, unsigned grid_y, unsigned grid_z,
                   unsigned block_x, unsigned block_y, unsigned block_z, void **args,
                   size_t shared_bytes, ststhip_stream stream);

/* Workgroups of `block_threads` threads of kernel `function` that one CU keeps resident (HIP
 * occupancy query); the sweep launcher sizes its wave grid in whole residency rounds with it. */
int ststhip_occupancy(const void *function, unsigned block_threads, size_t shared_bytes,
                      int *blocks_per_cu);

/* Bytes of scratch (private memory: register spills, dynamically indexed locals) per work-item of kernel
 * `function`, from the code object.  The C++ templates use it to leave out temporal-blocking depths whose kernel the
 * compiler could only build with spills (hip/StencilUpdate.hpp: a user's transition function may need far more
 * registers than its cell size suggests). */
int ststhip_kernel_scratch_bytes(const void *function, size_t *bytes_per_work_item);

/* How many sweep launches the pass driver currently keeps in flight side by side (1 outside of
 * ststhip_run_passes).  The launcher sizes its row chunks with it: concurrent launches share the
 * chip and hide each other's tails, so longer chunks (fewer warm-up rows) pay. */
int ststhip_launch_concurrency(void);
/* 1 while the pass driver is in a pass whose target planes were already written, row for row, by the pass
 * before the previous one of the same call (the third pass of a run and every later one); 0 otherwise.  The
 * sweep launcher then leaves out the stores of the per-field planes a transition function declares constant
 * (F::constant_fields): they already hold those values. */
int ststhip_target_holds_constants(void);
/* The device table of time-dependent values the pass driver has built for the call it is in (ststhip_sweep_desc:
 * tdv_size / fill_tdv / tdv_device_table), for the calling thread: `base` = value of generation `first_iteration`,
 * `n_values` of `value_size` bytes; base = NULL outside of such a call.  The sweep launcher points the kernel at it
 * instead of evaluating the launch's values on the host (tdv::single_pass strategies, hip/StencilUpdate.hpp). */
int ststhip_current_tdv_table(const void **base, uint64_t *first_iteration, uint64_t *n_values,
                              uint64_t *value_size);
/* A host that runs row-range sweeps side by side itself (the multi-GPU strip driver,
 * stencilstream_amd/dist.py) states their number here for the calling thread; 1 resets it. */
int ststhip_set_launch_concurrency(int n_launches_side_by_side);
/* A hole in the row range of the calling thread's next sweep launches: rows [*begin, *end) are left out, the
 * launch produces the rows on both sides of them (begin == end: no hole, the state outside of a driver).  The
 * strip driver sweeps the two boundary bands of a strip as one launch this way -- one dependent chain of band
 * latency per pass instead of two (ststhip_strip_advance).  The setter is for hosts that drive ststhip_app_sweep
 * themselves: set it, launch over [top of the upper band, end of the lower band), reset it with (0, 0). */
int ststhip_launch_row_hole(uint64_t *begin, uint64_t *end);
int ststhip_set_launch_row_hole(uint64_t begin, uint64_t end);
/* The global columns [begin, end) the calling thread's next sweep launches produce (begin == end: all columns the
 * buffers hold inside the grid, the state outside of a driver).  The block driver (ststhip_block_*) names the owned
 * columns of a block, widened by what the rest of a launch group still needs, this way; the row range stays an
 * argument of the launch.  Every launch through hip/internal/Sweep.hpp's launch_sweep honours it. */
int ststhip_launch_columns(uint64_t *begin, uint64_t *end);
int ststhip_set_launch_columns(uint64_t begin, uint64_t end);
/* Into how many row strips (1 or 2) a caller that advances `rows` x `width` cells of `app` for
 * `n_passes` launches should split them, each strip on its own stream and coupled to its
 * neighbours through halo-deep boundary bands only: the rule ststhip_run_passes applies to a whole
 * grid, for callers that drive ststhip_app_sweep themselves.  Returns 1 for unknown apps. */
int ststhip_suggest_row_strips(const char *app, uint64_t rows, uint64_t width, uint64_t n_passes);

/* Tuning knobs of the launcher and the drivers.  They come from the environment (STSTHIP_<NAME>, upper case) ONCE,
 * when the runtime first needs them (ststhip_init), never per launch; a host that changes its environment afterwards
 * (tools, tests) calls ststhip_reload_options().  0 / -1 = "not set, use the built-in rule" where noted.  Every knob
 * changes speed only, never results. */
typedef struct {
    int32_t chunk_rows;            /* rows of output per wave; 0 = the launcher's rule                    */
    int32_t tail_permille;         /* weight of a launch's ragged tail in that rule; 0 = built-in         */
    int32_t n_taper;               /* entries of STSTHIP_TAPER="permille:split,..."; -1 = built-in        */
    int32_t taper_permille[3], taper_split[3];
    int32_t narrow_form_kcells;    /* grids up to this many thousand cells run the one-cell-per-lane form */
    int32_t narrow_band_rows;      /* so do launches of at most this many rows (0 = never)                */
    int32_t skip_constant_stores;  /* leave out the stores of F::constant_fields where the target holds them */
    int32_t xcd_remap, last_chunk_early;
    int32_t max_generations;       /* cap of the temporal-blocking depth; 0 = the compiled maximum        */
    int32_t allow_spilling_depths; /* C++ templates: also use depths whose kernel spills registers        */
    int32_t virtual_strips;        /* row strips of the pass driver; 0 = its rule                         */
    int32_t two_strips_permille, two_strips_permille_outer; /* thresholds of that rule                    */
    int32_t strip_skew_permille;   /* where the pass driver cuts two strips; 0 = built-in                 */
    int32_t bands_beside_interior, band_stream_priority, bands_apart, bands_one_launch, comm_stream_priority;
    int32_t jacobi_fastpath, conway_fastpath;
    int32_t prepare_streams;       /* create and first-use the pass driver's streams at ststhip_init      */
    int32_t host_cache_mib;        /* free pinned host blocks kept for reuse                              */
    int32_t tune_depth;            /* pass driver, families with two candidate depths (ststhip_sweep_desc::alt_generations):
                                      1 (default) = time both on the first long call for a grid shape and keep the faster;
                                      0 = always the trusted depth; N >= 2 = depth N outright                         */
    int32_t exchange_every;        /* strip driver: exchange m*g ghost rows every m-th launch; 0/1 = every launch */
    int32_t stream_upload;         /* 1 (default) = a grid that is not in HBM yet is uploaded in row blocks and the pass
                                      driver starts on the blocks that have arrived (ststhip_set_source_arrival); 0 = one
                                      copy in front of the first pass                                                   */
    int32_t upload_block_mib;      /* size of those blocks; 0 = the rule of ststhip_suggest_upload_blocks              */
    int32_t skewed_strips;         /* pass driver, two row strips: 1 (default) = their common boundary moves up by a launch's
                                      ghost rows from pass to pass (no boundary bands: one launch per strip and pass, the
                                      upper strip never waits for the lower one); 0 = fixed strips with boundary bands on
                                      streams of their own (rounds 1-3)                                                   */
    int32_t strip_substrips;       /* strip driver: a rank's strip as two sub-strips with a moving boundary (two launches in
                                      flight); -1 (default) = the rule of ststhip_suggest_row_strips on the strip's cells,
                                      1 = never, 2 = wherever the strip is tall enough                                  */
    int32_t reserved[3];
} ststhip_options;
const ststhip_options *ststhip_get_options(void);
int ststhip_reload_options(void);

/* AoS <-> per-field planes by byte geometry (the reference's scatter/gather kernels,
 * StencilStream/cuda/StencilUpdate.hpp:294-321 and :408-438).  Field f of cell i is the
 * `field_size[f]` bytes at aos + i*cell_size + field_offset[f]; plane f holds them densely.
 * Staged through LDS so that both the AoS side and the plane side move whole cache lines. */
int ststhip_scatter_fields(const void *aos, size_t cell_size, size_t n_cells, int n_fields,
                           const size_t *field_offset, const size_t *field_size,
                           void *const *planes, ststhip_stream stream);
int ststhip_gather_fields(void *aos, size_t cell_size, size_t n_cells, int n_fields,
                          const size_t *field_offset, const size_t *field_size,
                          const void *const *planes, ststhip_stream stream);

/* Device-side maximum of |field| over a sub-rectangle of an AoS grid, for up to 8 fields in ONE pass over the
 * cells: what an application's convergence check needs from a grid without bringing the cells to the host
 * (replaces the host scan of examples/convection/convection.cpp:412-438; an extension -- the reference's API has
 * no reduction).  Field i is the f32 / f64 at byte `offset` of every cell; only cells with row < row_limit and
 * column < col_limit count.  result[i] = max |value| (NaNs are skipped, as `std::abs(v) > max` skips them), or
 * -infinity when no cell counts.  Wave-level DPP reduction, one atomic per wave and field.  Synchronises
 * `stream` and writes `result` (host memory) before returning. */
#define STSTHIP_F32 0u
#define STSTHIP_F64 1u
typedef struct {
    uint32_t offset;
    uint32_t type; /* STSTHIP_F32 or STSTHIP_F64 */
    uint64_t row_limit;
    uint64_t col_limit;
} ststhip_reduce_field;
int ststhip_reduce_max_abs(const void *cells, size_t cell_size, uint64_t height, uint64_t width,
                           uint64_t pitch, int n_fields, const ststhip_reduce_field *fields,
                           double *result, ststhip_stream stream);

/* Device-side norms of up to 8 fields of a grid, or of the difference of two grids of the same layout: what "has the
 * grid stopped changing", an L2 norm, a conservation check and "has anything become NaN" need, in one read of the
 * cells at HBM speed (an extension, as ststhip_reduce_max_abs; additive within ABI 6).
 *
 * A field is the f32 / f64 of cell (row r, column c) at  base + (r * pitch + c) * stride  bytes: a member of an AoS cell
 * (base = cells + offset of the member, stride = sizeof(Cell)) and a per-field plane (stride = size of the element;
 * the planes of ststhip_app_run and ststhip_strip_plane) alike.  It is reduced over the rectangle
 * [row_begin, row_end) x [col_begin, col_end), clipped to height x width; the rectangle may be empty.
 *
 * Every element is converted to double; the per-cell value v is the element of a (ststhip_grid_norms) or
 * double(a) - double(b), one rounding (ststhip_grid_distance: other_base[i] is the base of field i in the second grid,
 * same stride, pitch and rectangle).  Cells whose v is NaN or +-infinity are counted in n_nonfinite and take part in
 * nothing else.
 *
 * No floating-point atomics: a lane accumulates in double, the 64 lanes of a wave and then the waves of a workgroup
 * combine in a fixed order, every workgroup writes one partial per field and quantity and a second kernel adds the
 * partials in index order.  The number of workgroups depends on the rectangle and the layout only, so the same call on
 * the same data returns the same bits every time, on every device.
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID: n_fields outside 1..8, an unknown
 * type, stride 0, a base or stride that is no multiple of the element's size, pitch < width, a null base with a
 * non-empty rectangle).  Ordered on `stream`; synchronises it and writes `result` (host memory) before returning. */
typedef struct {
    const void *base;   /* the field's element of cell (0, 0)                              */
    uint64_t stride;    /* bytes between neighbouring cells of a row                       */
    uint64_t pitch;     /* cells between neighbouring rows (>= width)                      */
    uint64_t height;    /* extents of the grid the rectangle is clipped to                 */
    uint64_t width;
    uint64_t row_begin, row_end, col_begin, col_end;
    uint32_t type;      /* STSTHIP_F32 or STSTHIP_F64                                      */
    uint32_t reserved;  /* 0                                                               */
} ststhip_norm_field;
typedef struct {
    uint64_t n_cells;     /* cells of the clipped rectangle                                */
    uint64_t n_nonfinite; /* of these, cells whose v is NaN or +-infinity                  */
    double max_abs;       /* max |v| over the finite v, exact; -infinity if there is none  */
    double sum;           /* sum of v, of |v| and of v*v over the finite v, in double      */
    double sum_abs;
    double sum_sq;
} ststhip_norm_result;
int ststhip_grid_norms(int n_fields, const ststhip_norm_field *fields, ststhip_norm_result *result,
                       ststhip_stream stream);
int ststhip_grid_distance(int n_fields, const ststhip_norm_field *fields, const void *const *other_base,
                          ststhip_norm_result *result, ststhip_stream stream);

/* Grid regions: move a rectangle of a grid, or of one member of its cells, where the cells are -- device to device,
 * a constant into a rectangle, or between HBM and host memory without the rest of the grid (an extension, as the
 * norms; additive within ABI 6).  What a host that looks at its grid or nudges it between two updates needs: one
 * member of every cell for a frame (optionally every k-th row and column), a source injected into a handful of cells.
 *
 * A view is the byte geometry of ststhip_norm_field: the element of cell (r, c) is the `elem_size` bytes at
 * base + (r * pitch + c) * stride.  A member of an AoS cell (base = cells + offset of the member, stride =
 * sizeof(Cell)), a whole cell (elem_size = stride = sizeof(Cell)), a per-field plane (stride = elem_size), a grid of
 * bools and host memory with any row pitch are all views.  Bytes are moved verbatim: NaN payloads, signed zeros and
 * padding the caller names arrive unchanged.  Nothing needs to be aligned: base, stride and elem_size are arbitrary,
 * the kernels pick the widest access all of them allow and the result is the same for every width.
 *
 * Element (i, j) of the n_rows x n_cols rectangle is read from source cell (src_row + i * src_row_step,
 * src_col + j * src_col_step) and lands in destination cell (dst_row + i, dst_col + j).  Nothing is clipped: a
 * rectangle that leaves its view is an error.  An empty rectangle (n_rows == 0 or n_cols == 0) succeeds on the host,
 * also with a null base and without a device.
 *
 * One to eight entries per call.  The entries of one call run in NO particular order and are not checked against each
 * other: a caller must not let one entry write what another entry reads or writes.
 *
 * Limits, so that a lane's offset inside a row fits 32 bits: n_rows and n_cols are below 2^31, and so is the byte extent
 * of a rectangle's row in either view, n_cols * src_col_step * src.stride and n_cols * dst.stride.
 *
 * Source and destination of one entry may share memory in one way only.  If the byte spans of the two rectangles
 * (first byte of the first element to last byte of the last) intersect, the entry is accepted only when both views
 * have the same stride and pitch, both steps are 1 and the destination's first element lies d bytes behind or in front
 * of the source's with elem_size <= d and d + elem_size <= stride: one member of a cell copied to another member of
 * the same cells.  Everything else that intersects is refused.
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid region"): n outside 1..8, elem_size outside 1..128 or above a stride, stride 0, pitch < width, a step of 0, a
 * null base with a non-empty rectangle, a null `value`, extents that describe more than 2^63 bytes, a rectangle outside
 * its view, the limits and the overlap rule above.
 *
 * ststhip_grid_copy (device to device) and ststhip_grid_fill are ordered on `stream` and do not synchronise;
 * `value` is read inside the call.  ststhip_grid_download packs the rectangle on the device into pooled staging,
 * copies that to the host and synchronises `stream` before it returns; dst is host memory, dense within a row
 * (dst.stride == elem_size), rows dst.pitch elements apart.  ststhip_grid_upload is its mirror: src is host memory
 * (src.stride == elem_size, both steps 1, any pitch), copied to pooled staging and unpacked from there; it
 * synchronises `stream`, so the caller's buffer is free on return. */
typedef struct {
    void *base;        /* the element of cell (0, 0)                         */
    uint64_t stride;   /* bytes between neighbouring cells of a row          */
    uint64_t pitch;    /* cells between neighbouring rows (>= width)         */
    uint64_t height, width;
} ststhip_grid_view;
typedef struct {
    ststhip_grid_view dst, src;
    uint32_t elem_size;              /* bytes moved per cell, 1 .. 128        */
    uint32_t reserved;               /* 0                                     */
    uint64_t dst_row, dst_col;       /* where element (0, 0) of the rectangle lands */
    uint64_t src_row, src_col;       /* the first cell read                   */
    uint64_t n_rows, n_cols;         /* elements moved per axis               */
    uint64_t src_row_step, src_col_step; /* >= 1: element (i, j) comes from source cell
                                        (src_row + i*row_step, src_col + j*col_step) */
} ststhip_grid_copy_desc;
typedef struct {
    ststhip_grid_view dst;
    uint32_t elem_size, reserved;
    uint64_t dst_row, dst_col, n_rows, n_cols;
    const void *value;               /* elem_size bytes, host memory, read inside the call */
} ststhip_grid_fill_desc;
int ststhip_grid_copy(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream);
int ststhip_grid_fill(int n, const ststhip_grid_fill_desc *fills, ststhip_stream stream);
int ststhip_grid_download(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream);
int ststhip_grid_upload(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream);

/* Grid algebra: linear combinations of a few grids and the 2:1 transfer between a fine and a coarse grid, computed
 * where the cells are (an extension, as the norms and the regions; additive within ABI 6).  What turns a smoother into
 * a solver between two update calls: a weighted correction u <- (1-w) u + w J(u), a residual, a multigrid cycle
 * u <- u + P(e).  Views are ststhip_grid_view, elements are STSTHIP_F32 or STSTHIP_F64: planes and members of AoS
 * cells alike.
 *
 * The results are DEFINED OPERATION BY OPERATION: every multiplication and every addition below is done in the
 * element's own type, rounded once, evaluated left to right and never fused (the library is built with
 * -ffp-contract=off), so numpy in the same dtype is a bit-exact model.  Subnormal results are kept, not flushed.
 *
 * ststhip_grid_combine, element by element over the n_rows x n_cols rectangle: x_k is the element of term k's view at
 * (term[k].row + i, term[k].col + j), the result lands in the destination at (dst_row + i, dst_col + j):
 *     acc = coef_0 * x_0;  then for k = 1 .. n_terms-1:  acc = acc + coef_k * x_k.
 * Coefficients are converted from double to the element's type once, on the host.  (A constant offset: ststhip_grid_fill,
 * then a combine.)
 *
 * ststhip_grid_resample: grids are cell-centred, H x W cells with a halo outside; n_rows and n_cols count COARSE cells
 * in both modes.
 *   STSTHIP_RESTRICT_MEAN: the destination is coarse; with s(a, b) = source cell (src_row + a, src_col + b)
 *     dst(dst_row+i, dst_col+j) = ((s(2i,2j) + s(2i,2j+1)) + (s(2i+1,2j) + s(2i+1,2j+1))) * 0.25
 *   in exactly this order.  The 2 n_rows x 2 n_cols source rectangle lies inside its view; src_row / src_col may be odd.
 *   STSTHIP_PROLONG_BILINEAR: the destination is fine; for coarse cell (i, j) of the rectangle and a, b in {0, 1} the
 *   fine cell (dst_row + 2i + a, dst_col + 2j + b) gets
 *     h(r) = 0.75 * c(r, j) + 0.25 * c(r, j_far)      j_far = j - 1 for b = 0, j + 1 for b = 1
 *     v    = 0.75 * h(i)    + 0.25 * h(i_far)         i_far = i - 1 for a = 0, i + 1 for a = 1
 *   where c(r, q) is source cell (src_row + r, src_col + q), every product and every sum rounded once.  A neighbour
 *   outside the source VIEW reads `halo`, converted to the element's type (the meaning of Params::halo_value); one
 *   outside the rectangle but inside the view reads the view, so that tiles and strips compose.
 *
 * As for the regions: one to eight entries per call, run in NO particular order and not checked against each other;
 * nothing is clipped; an empty rectangle (n_rows == 0 or n_cols == 0) succeeds on the host, also with null bases and
 * without a device; n_rows, n_cols and the byte extent of a rectangle's row in every view are below 2^31 (for a
 * resample the fine side counts).  Unlike the regions, and as for the norms, base and stride are multiples of the
 * element's size.  Calls are ordered on `stream` and do not synchronise.
 *
 * Overlap.  A term of a combine whose byte span (first byte of its rectangle's first element to the last byte of the
 * last) intersects the destination's is accepted in two cases only: the term IS the destination (same first-element
 * address, stride and pitch; a lane reads its own element before it writes it), or it is another member of the same
 * cells by the regions' rule (same stride and pitch, first elements d bytes apart with elem_size <= d and
 * d + elem_size <= stride).  A resample refuses any intersection of the destination's span with the span of what it
 * reads (for a prolongation the neighbours inside the view included).
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid algebra"): n outside 1..8, n_terms outside 1..4, an unknown type or mode, stride 0, pitch < width, a null base
 * with a non-empty rectangle, misalignment, extents that describe more than 2^63 bytes, a rectangle outside its view,
 * the limits and the overlap rules above. */
#define STSTHIP_RESTRICT_MEAN 0u
#define STSTHIP_PROLONG_BILINEAR 1u
typedef struct {
    ststhip_grid_view src;
    uint64_t row, col;               /* where element (0, 0) of the rectangle is read */
    double coef;
} ststhip_grid_term;
typedef struct {
    ststhip_grid_view dst;
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64            */
    uint32_t n_terms;                /* 1 .. 4                                */
    uint64_t dst_row, dst_col;       /* where element (0, 0) of the rectangle lands */
    uint64_t n_rows, n_cols;
    ststhip_grid_term term[4];
} ststhip_grid_combine_desc;
typedef struct {
    ststhip_grid_view dst, src;
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64            */
    uint32_t mode;                   /* STSTHIP_RESTRICT_MEAN or STSTHIP_PROLONG_BILINEAR */
    uint64_t dst_row, dst_col;       /* the first cell written                */
    uint64_t src_row, src_col;       /* the first cell of the source rectangle */
    uint64_t n_rows, n_cols;         /* COARSE cells per axis, in both modes  */
    double halo;                     /* prolong: what a neighbour outside the source view reads */
} ststhip_grid_resample_desc;
int ststhip_grid_combine(int n, const ststhip_grid_combine_desc *combines, ststhip_stream stream);
int ststhip_grid_resample(int n, const ststhip_grid_resample_desc *resamples, ststhip_stream stream);

/* Grid stencils: a 3 x 3 linear operator applied to a grid once, with an optional right-hand side (an extension, as
 * the algebra; additive within ABI 6).  The piece of the routes above that reads neighbours: a residual r = f - A u is
 * weight = -A, rhs_coef = 1; a Poisson relaxation u <- 1/4 (N + W + E + S) + 1/4 h^2 f is
 * weight = {0, 1/4, 0,  1/4, 0, 1/4,  0, 1/4, 0}, rhs_coef = 1/4 h^2.  Views and element types are the algebra's.
 *
 * The result is DEFINED OPERATION BY OPERATION, as the algebra's.  For element (i, j) of the n_rows x n_cols rectangle
 * let s(a, b) be source cell (src_row + i + a, src_col + j + b).  The taps of the shape are taken in row-major order,
 *     BOX9:   (-1,-1) (-1,0) (-1,+1) (0,-1) (0,0) (0,+1) (+1,-1) (+1,0) (+1,+1)
 *     CROSS5: (-1,0) (0,-1) (0,0) (0,+1) (+1,0)
 * and with w(a, b) = weight[3 * (a + 1) + (b + 1)]
 *     acc = w_first * s_first;   then, for every further tap in that order:   acc = acc + w_k * s_k;
 *     if has_rhs:                acc = acc + rhs_coef * rhs(rhs_row + i, rhs_col + j);
 *     dst(dst_row + i, dst_col + j) = acc
 * Every product and every sum is rounded once in the element's type and never fused; subnormals are kept.  Weights,
 * rhs_coef and halo are converted from double once, on the host.  EVERY tap of the shape is multiplied, also one whose
 * weight is zero: 0 * inf is NaN, as in numpy.  The four corner taps of CROSS5 are neither read nor multiplied; a
 * CROSS5 entry whose corner weights are not +0.0 or -0.0 is refused.  A neighbour outside the source VIEW reads `halo`
 * (the meaning of Params::halo_value); one outside the rectangle but inside the view reads the view, so that tiles and
 * strips compose, as for STSTHIP_PROLONG_BILINEAR.
 *
 * The conventions are the algebra's: one to eight entries per call, run in NO particular order and not checked against
 * each other; nothing is clipped; an empty rectangle succeeds on the host, also with null bases and without a device;
 * n_rows, n_cols and the byte extent of a rectangle's row in every view are below 2^31; bases and strides are
 * multiples of the element's size; the call is ordered on `stream` and does not synchronise.
 *
 * Overlap.  What the stencil reads is the rectangle widened by one cell on every side where that lies inside the view.
 * The byte span of that may intersect the destination's span in one case only: src is another member of the
 * destination's cells by the regions' rule (same stride and pitch, the first elements of the two rectangles d bytes
 * apart with elem_size <= d and d + elem_size <= stride); a lane then never writes bytes that another lane reads.  src
 * being the destination itself is refused: a stencil in place is a race.  rhs follows the rule of a combine's term: it
 * may BE the destination (same first-element address, stride and pitch; a lane reads its own element before it writes
 * it) or another member of the same cells; every other intersection is refused.
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid stencil"): n outside 1..8, an unknown type or shape, reserved != 0, stride 0, pitch < width, a null base with a
 * non-empty rectangle, misalignment, extents that describe more than 2^63 bytes, a rectangle outside its view, a weight
 * or (with has_rhs) an rhs_coef that is not finite (a halo may be anything), non-zero corner weights with CROSS5, the
 * limits and the overlap rules above.  With has_rhs == 0, rhs, rhs_row, rhs_col and rhs_coef are ignored. */
#define STSTHIP_STENCIL_CROSS5 0u     /* taps N, W, C, E, S                    */
#define STSTHIP_STENCIL_BOX9 1u       /* all nine taps                         */
typedef struct {
    ststhip_grid_view dst, src, rhs; /* rhs is ignored (may be all zero) when has_rhs == 0 */
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64            */
    uint32_t shape;                  /* STSTHIP_STENCIL_CROSS5 or STSTHIP_STENCIL_BOX9 */
    uint32_t has_rhs, reserved;      /* reserved = 0                          */
    uint64_t dst_row, dst_col;       /* where element (0, 0) of the rectangle lands */
    uint64_t src_row, src_col;       /* the centre tap of element (0, 0)      */
    uint64_t rhs_row, rhs_col;       /* where element (0, 0) of the right-hand side is read */
    uint64_t n_rows, n_cols;
    double weight[9];                /* row-major: weight[3*(a+1) + (b+1)] multiplies src(i+a, j+b) */
    double rhs_coef;
    double halo;                     /* what a neighbour outside the source view reads */
} ststhip_grid_stencil_desc;
int ststhip_grid_stencil(int n, const ststhip_grid_stencil_desc *stencils, ststhip_stream stream);

/* Grid inner products: sum a*b over a rectangle of two grids, with sum a*a and sum b*b of the same cells (an extension,
 * as the norms and the algebra; additive within ABI 6).  What the routes above lack for a Krylov method: <p, A p> of
 * conjugate gradients, a steepest-descent step length, a projection, the cosine between two fields.  Views and element
 * types are the algebra's: planes and members of AoS cells alike; a and b have their own stride and pitch each, so a
 * plane against a member of struct cells is one call.
 *
 * Element (i, j) of the n_rows x n_cols rectangle is read from cell (a_row + i, a_col + j) of a and from cell
 * (b_row + i, b_col + j) of b.  Per cell x = double(a), y = double(b).  A cell where x or y is NaN or +-infinity is
 * counted in n_nonfinite, once, and takes part in nothing else.  Every other cell adds x*y to dot, x*x to sum_aa and
 * y*y to sum_bb: every product and every sum is rounded once in double and never fused.  The products of f32 elements
 * are exact in double.  Sums of finite f64 products may overflow to infinity; that is the caller's, as for sum_sq of
 * the norms.
 *
 * The conventions are the algebra's, not the norms': nothing is clipped, a rectangle that leaves either view is an
 * error; an empty rectangle (n_rows == 0 or n_cols == 0) succeeds on the host with an all-zero result, also with null
 * bases and without a device; n_rows, n_cols and the byte extent of a rectangle's row in either view are below 2^31;
 * bases and strides are multiples of the element's size; one to eight entries per call, result[i] belongs to pairs[i].
 *
 * Everything is only read, so a and b may overlap in any way.  Where they are the same cells (a == b), dot, sum_aa and
 * sum_bb are the same bits.  Exchanging a and b of an entry exchanges sum_aa and sum_bb and leaves dot's bits alone:
 * which cells a lane takes, and in which order, depends on the two sides alike (the rectangle, whether both are dense
 * within a row, and how the two sit relative to a 16-byte boundary), never on which of them is called a.
 *
 * No floating-point atomics: a lane accumulates in double over the cells it owns, the 64 lanes of a wave and then the
 * waves of a workgroup combine in a fixed order, every workgroup writes one partial per quantity and a second kernel
 * adds the partials in index order.  The number of workgroups depends on the rectangle and on the two layouts (dense or
 * strided) only, never on the device or an occupancy query, so the same call on the same data returns the same bits
 * every time, on every device (of the addresses only their position relative to a 16-byte boundary belongs to "the
 * same call": it decides where a dense row's 16-byte loads begin, as for the norms).
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid dot"): n outside 1..8, a null `pairs` or `result`, an unknown type, reserved != 0, stride 0, pitch < width,
 * misalignment, a null base with a non-empty rectangle, extents that describe more than 2^63 bytes, a rectangle outside
 * a view and the limits above.  Ordered on `stream`; synchronises it and writes `result` (host memory) before
 * returning, like the norms. */
typedef struct {
    ststhip_grid_view a, b;          /* const in effect; bases are only read  */
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64, of both sides */
    uint32_t reserved;               /* 0                                     */
    uint64_t a_row, a_col;           /* where element (0, 0) of the rectangle is read in a */
    uint64_t b_row, b_col;           /* ... and in b                          */
    uint64_t n_rows, n_cols;
} ststhip_grid_dot_desc;
typedef struct {
    uint64_t n_cells;                /* n_rows * n_cols                       */
    uint64_t n_nonfinite;            /* cells where x or y is NaN or +-infinity */
    double dot;                      /* sum of x*y over the other cells, in double */
    double sum_aa, sum_bb;           /* sum of x*x and of y*y over the same cells */
} ststhip_grid_dot_result;
int ststhip_grid_dot(int n, const ststhip_grid_dot_desc *pairs, ststhip_grid_dot_result *result,
                     ststhip_stream stream);

/* Grid relaxation: red-black sweeps of the five-point operator IN PLACE (an extension, as the stencils; additive within
 * ABI 6).  The smoother of a multigrid cycle without a second grid: ststhip_grid_stencil refuses src == dst, because a
 * stencil in place is a race; a cell of one colour has only neighbours of the other colour, so updating one colour at
 * a time is race-free by construction and the result is one defined set of bits.  Views and element types are the
 * algebra's.
 *
 * Colour.  The colour of cell (r, q) in VIEW coordinates is (r + q + parity) & 1.  It does not depend on the
 * rectangle, so tiles of one grid agree; a rank of a strip run passes the parity of its first row's global index.
 *
 * Half-sweeps.  Half-sweep k, for k = 0 .. n_half_sweeps - 1, updates exactly the cells of the n_rows x n_cols
 * rectangle (from (u_row, u_col) on) whose colour is (first_colour + k) & 1; a full Gauss-Seidel sweep is
 * n_half_sweeps = 2.  The half-sweeps of one entry are ordered among themselves.
 *
 * The update is DEFINED OPERATION BY OPERATION and is exactly the stencil's CROSS5.  For such a cell (u_row + i,
 * u_col + j) with its neighbours N (row - 1), W (column - 1), C (itself), E (column + 1), S (row + 1):
 *     acc = w_n * N;  acc = acc + w_w * W;  acc = acc + w_c * C;  acc = acc + w_e * E;  acc = acc + w_s * S;
 *     if has_rhs:     acc = acc + rhs_coef * rhs(rhs_row + i, rhs_col + j);
 *     u(u_row + i, u_col + j) = acc
 * with weight = {w_n, w_w, w_c, w_e, w_s}.  Every product and every sum is rounded once in the element's type and
 * never fused; subnormals are kept.  Weights, rhs_coef and halo are converted from double once, on the host.  EVERY
 * tap is multiplied, also one whose weight is zero: 0 * inf is NaN, as in numpy.  A neighbour outside the VIEW reads
 * `halo`; one outside the rectangle but inside the view reads the view and is never written by this entry, so that
 * tiles and strips compose.  All four neighbours have the other colour: a half-sweep reads only values that the
 * previous half-sweep left.  Cells of the other colour, and everything outside the rectangle, keep their bytes.
 * SOR with factor omega for (4 u - N - W - E - S) / h^2 = f is weight = {omega/4, omega/4, 1 - omega, omega/4,
 * omega/4}, rhs_coef = omega h^2 / 4; omega = 1 is Gauss-Seidel.
 *
 * The conventions are the stencil's: one to eight entries per call, run in NO particular order and not checked against
 * each other (two entries that touch each other's cells are the caller's problem); nothing is clipped; an empty
 * rectangle succeeds on the host, also with null bases and without a device; n_rows, n_cols and the byte extent of a
 * rectangle's row in either view are below 2^31; bases and strides are multiples of the element's size; the call is
 * ordered on `stream` and does not synchronise.
 *
 * Overlap.  What the entry reads or writes of u is the rectangle widened by one cell on every side where that lies
 * inside the view.  rhs may be another member of u's cells by the regions' rule (same stride and pitch, the first
 * elements of the two rectangles d bytes apart with elem_size <= d and d + elem_size <= stride).  Every other
 * intersection of rhs's byte span with that of the widened rectangle is refused, rhs being u itself included.
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid relax"): n outside 1..8, an unknown type, first_colour or parity above 1, n_half_sweeps outside 1..1024,
 * reserved != 0, stride 0, pitch < width, a null base with a non-empty rectangle, misalignment, extents that describe
 * more than 2^63 bytes, a rectangle outside its view, a weight or (with has_rhs) an rhs_coef that is not finite (a halo
 * may be anything), the limits and the overlap rule above.  With has_rhs == 0, rhs, rhs_row, rhs_col and rhs_coef are
 * ignored. */
typedef struct {
    ststhip_grid_view u, rhs;        /* u is read and written; rhs ignored when has_rhs == 0 */
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64            */
    uint32_t has_rhs;
    uint32_t first_colour;           /* 0 or 1: the colour of half-sweep 0    */
    uint32_t n_half_sweeps;          /* 1 .. 1024, run in order, colours alternating */
    uint32_t parity, reserved;       /* parity 0 or 1; reserved = 0           */
    uint64_t u_row, u_col;           /* the rectangle's first cell in u       */
    uint64_t rhs_row, rhs_col;       /* where element (0, 0) of the right-hand side is read */
    uint64_t n_rows, n_cols;
    double weight[5];                /* n, w, c, e, s -- Cross5's order       */
    double rhs_coef;
    double halo;                     /* what a neighbour outside the view of u reads */
} ststhip_grid_relax_desc;
int ststhip_grid_relax(int n, const ststhip_grid_relax_desc *relaxations, ststhip_stream stream);

/* Grid diffusion: the five-point finite-volume operator whose weights are FACE COEFFICIENTS STORED IN TWO GRIDS (an
 * extension, as the stencils; additive within ABI 6).  ststhip_grid_stencil and ststhip_grid_relax take constant weights;
 * this is the variable-coefficient operator A u = sigma u - scale div(k grad u): heterogeneous conduction, an implicit
 * heat step (sigma + A) u = b, masked domains, Neumann walls.  kx holds the EAST face of every cell, ky its SOUTH face,
 * so the operator is symmetric by construction; a zero face is an insulated wall, a ring of zero faces cuts a cell out.
 * Three modes: apply (a residual, CG's A p), one damped Jacobi step (a smoother that needs no colouring) and the diagonal
 * solve z = r / diag(A) (the Jacobi preconditioner).  Views and element types are the algebra's.
 *
 * The result is DEFINED OPERATION BY OPERATION, as the stencil's.  For element (i, j) of the n_rows x n_cols rectangle
 * let X(a, b) be view X at (X_row + i + a, X_col + j + b):
 *     c = u(0,0), n = u(-1,0), w = u(0,-1), e = u(0,+1), s = u(+1,0)
 *     ke = kx(0,0) (this cell's east face), kw = kx(0,-1) (the west neighbour's east face),
 *     ks = ky(0,0) (this cell's south face), kn = ky(-1,0) (the north neighbour's south face), f = rhs(0,0)
 * A neighbour outside u's VIEW reads `halo`, one outside the rectangle but inside the view reads the view.  kw outside
 * kx's view and kn outside ky's view read `k_halo`; every view is judged by its own extents.  Then
 *     acc = kn*(c-n);  acc = acc + kw*(c-w);  acc = acc + ke*(c-e);  acc = acc + ks*(c-s)
 *     d = kn + kw;  d = d + ke;  d = d + ks;  d = scale*d;  d = sigma + d
 *     APPLY:       y = sigma*c;  y = y + scale*acc;  if has_rhs:  y = y + rhs_coef*f
 *     JACOBI:      t = sigma*c;  t = t + scale*acc;  r = rhs_coef*f;  r = r - t;  y = c + omega*(r/d)
 *     SOLVE_DIAG:  y = (rhs_coef*f)/d            (u is neither read nor validated)
 *     dst(0,0) = y
 * Every product, sum, difference and quotient is rounded once in the element's type and never fused; subnormals are
 * kept; `/` is the IEEE correctly rounded quotient, and a zero d gives what IEEE gives (+-inf, or NaN for 0/0).
 * sigma, scale, omega, rhs_coef, halo and k_halo are converted from double once, on the host.  A zero coefficient is
 * multiplied like every other: 0 * inf is NaN, as in numpy.  JACOBI and SOLVE_DIAG need a right-hand side.
 *
 * The conventions are the stencil's: one to eight entries per call, run in NO particular order and not checked against
 * each other; nothing is clipped; an empty rectangle succeeds on the host, also with null bases and without a device;
 * n_rows, n_cols and the byte extent of a rectangle's row in every view are below 2^31; bases and strides are
 * multiples of the element's size; the call is ordered on `stream` and does not synchronise.
 *
 * Overlap.  What is read is u's rectangle widened by one cell on every side where that lies inside u's view, kx's
 * rectangle widened by one cell to the west and ky's by one cell to the north, where their views go on.  The byte span of
 * each of those may intersect the destination's span in one case only: the view is another member of the destination's
 * cells by the regions' rule (same stride and pitch, the first elements of the two rectangles d bytes apart with
 * elem_size <= d and d + elem_size <= stride).  u (or kx, ky) being the destination itself is refused.  rhs may BE the
 * destination (same first-element address, stride and pitch) or another member of the same cells; every other
 * intersection is refused.  u, kx, ky and rhs are only read and may overlap each other in any way.
 *
 * Arguments are validated before anything touches the device (STSTHIP_ERR_INVALID, ststhip_last_error() starts with
 * "grid diffusion"): n outside 1..8, a null table, an unknown type or mode, reserved != 0, JACOBI or SOLVE_DIAG without a
 * right-hand side, stride 0, pitch < width, a null base with a non-empty rectangle, misalignment, extents that describe
 * more than 2^63 bytes, a rectangle outside its view, a sigma, scale, rhs_coef (with has_rhs) or omega (in JACOBI) that
 * is not finite (halo and k_halo may be anything), the limits and the overlap rules above.  With has_rhs == 0, rhs,
 * rhs_row, rhs_col and rhs_coef are ignored; omega is read in JACOBI only; u, u_row and u_col are ignored in SOLVE_DIAG. */
#define STSTHIP_DIFFUSION_APPLY 0u
#define STSTHIP_DIFFUSION_JACOBI 1u
#define STSTHIP_DIFFUSION_SOLVE_DIAG 2u
typedef struct {
    ststhip_grid_view dst, u, kx, ky, rhs; /* rhs ignored when has_rhs == 0; u ignored in SOLVE_DIAG */
    uint32_t type;                   /* STSTHIP_F32 or STSTHIP_F64            */
    uint32_t mode;                   /* STSTHIP_DIFFUSION_APPLY, _JACOBI or _SOLVE_DIAG */
    uint32_t has_rhs, reserved;      /* reserved = 0                          */
    uint64_t dst_row, dst_col;       /* where element (0, 0) of the rectangle lands */
    uint64_t u_row, u_col;           /* the centre of element (0, 0)          */
    uint64_t kx_row, kx_col;         /* its east face                         */
    uint64_t ky_row, ky_col;         /* its south face                        */
    uint64_t rhs_row, rhs_col;       /* where element (0, 0) of the right-hand side is read */
    uint64_t n_rows, n_cols;
    double sigma, scale;             /* A = sigma + scale * (sum of the face fluxes) */
    double omega;                    /* the damping of a JACOBI step; read there only */
    double rhs_coef;
    double halo;                     /* what a neighbour outside the view of u reads */
    double k_halo;                   /* what kw reads outside kx's view, kn outside ky's */
} ststhip_grid_diffusion_desc;
int ststhip_grid_diffusion(int n, const ststhip_grid_diffusion_desc *entries, ststhip_stream stream);

/* ------------------------------------------------------------- layer 1 */

/* Where a buffer sits inside the global grid.  A single-GPU grid has row_origin = 0 and
 * local_rows = global_height.  A row strip of a domain-decomposed grid holds its owned rows plus
 * ghost rows: buffer row 0 is global row `row_origin` (may be "negative" for the first strip:
 * rows before global row 0 are never read). */
typedef struct {
    uint64_t global_height; /* stencil.grid_range[0]                              */
    uint64_t global_width;  /* stencil.grid_range[1]                              */
    int64_t row_origin;     /* global row index of buffer row 0                   */
    uint64_t local_rows;    /* rows held by the buffers                           */
    uint64_t pitch;         /* elements between consecutive rows (>= the columns held) */
    /* ABI 5: a block of a 2-D decomposition holds a column range too.  local_cols = 0: whole rows (columns
     * 0 .. global_width, the case of everything above); else buffer column 0 is global column `col_origin` (may be
     * negative for the first block of a row: columns before global column 0 are never read) and the buffers hold
     * `local_cols` columns: the owned ones plus ghost columns on both sides. */
    int64_t col_origin;
    uint64_t local_cols;
} ststhip_domain;

/* Static description of a precompiled transition function. */
typedef struct {
    const char *name;
    uint32_t cell_size;          /* sizeof(Cell) of the AoS cell                         */
    uint32_t params_size;        /* sizeof of the transition function's parameter block  */
    uint32_t stencil_radius;
    uint32_t n_subiterations;
    uint32_t n_planes;           /* 1 = AoS sweep; >1 = one plane per field (SoA sweep)  */
    uint32_t plane_elem_size[16];
    uint32_t field_offset[16];   /* byte offset of each plane's field inside the cell    */
    uint32_t max_generations;    /* deepest temporal blocking compiled in                */
    uint32_t tdv_size;           /* 0 = no time-dependent value                          */
    uint32_t halo_depth_per_generation; /* ghost rows one generation consumes per side   */
    uint32_t strip_width;        /* columns one wavefront produces at max_generations (staged sweeps: its share of the workgroup's strip) */
    uint32_t cells_per_lane;     /* adjacent cells a lane holds per row (K)              */
    uint32_t prefetch_rows;      /* rows loaded ahead of the pipeline (P)                */
    uint32_t stages;             /* waves of a workgroup that share one column strip as a pipeline over the levels (1 = independent waves) */
    uint32_t default_generations; /* depth of launches nobody has measured (= max_generations unless the function's
                                     tuning compiles a deeper family than it trusts: ststhip_sweep_desc::alt_generations) */
} ststhip_app_info;

/* Largest scratch (private memory: register spills, dynamically indexed locals) per work-item over the kernels a
 * launch of `app` at depth `n_generations` may start (default shape, narrow form, constant-plane variant), from the
 * code object.  The shipped library has none at any depth (tests/test_parity_gpu.py asserts it). */
int ststhip_app_scratch_bytes(const char *app, uint32_t n_generations, size_t *bytes_per_work_item);

int ststhip_app_count(void);
int ststhip_app_info_at(int index, ststhip_app_info *info);
int ststhip_app_find(const char *name, ststhip_app_info *info);

/* Advance global rows [out_row_begin, out_row_end) by `n_generations` (max_generations or one of its
 * repeated halvings) generations in ONE kernel launch, reading `src` and writing `dst` (arrays of
 * n_planes device pointers with identical geometry `dom`).  Rows of `dst` outside the range are
 * not touched.  Input rows [out_row_begin - g, out_row_end + g) that lie inside the global grid
 * must be present in `src`, g = n_generations * halo_depth_per_generation.  `tf_params` is the
 * host-side parameter block of the transition function, `halo_cell` one AoS cell.  The
 * time-dependent values of generations `iteration .. iteration+n-1` are evaluated on the host
 * inside this call, once each (reference: StencilStream/cuda/StencilUpdate.hpp:224). */
int ststhip_app_sweep(const char *app, const void *tf_params, const void *halo_cell,
                      const ststhip_domain *dom, const void *const *src, void *const *dst,
                      uint64_t out_row_begin, uint64_t out_row_end, uint64_t iteration,
                      uint32_t n_generations, ststhip_stream stream);

/* Timing of one ststhip_app_run call. */
typedef struct {
    double walltime_s;        /* host wall clock around the whole call (incl. final sync)      */
    double kernel_time_s;     /* sum of sweep-kernel durations from HIP events (if profiling)  */
    uint64_t n_launches;      /* sweep kernels launched                                         */
    uint64_t n_processed_cells; /* n_iterations * H * W (sub-iterations not counted)           */
    uint64_t n_streamed_passes; /* ABI 6: passes that ran as row tiles behind a source still arriving
                                   (ststhip_set_source_arrival); 0 otherwise                              */
} ststhip_run_info;

/* cuda::StencilUpdate::operator() for a precompiled transition function: advance the whole
 * grid by n_iterations generations.  `src` is only read; `dst` receives the result; both are
 * arrays of n_planes device pointers of geometry `dom` (row_origin 0, local_rows = height).
 * Scratch planes come from the runtime's pool.  blocking != 0 synchronises the stream before
 * returning; profiling != 0 brackets every sweep kernel with HIP events.  n_iterations == 0
 * copies src to dst.
 * Two applications have a second, bit-identical form the call switches to on its own:
 * "jacobi5general" with five equal positive coefficients and a +0 halo (product-carrying form),
 * and "conway" with halo = false, width and pitch multiples of four and 4-byte aligned planes
 * (four cells per 32-bit word).  Cells of "conway" are C++ bools: bytes 0 or 1, nothing else. */
int ststhip_app_run(const char *app, const void *tf_params, const void *halo_cell,
                    const ststhip_domain *dom, const void *const *src, void *const *dst,
                    uint64_t iteration_offset, uint64_t n_iterations, int blocking,
                    int profiling, ststhip_stream stream, ststhip_run_info *info);

/* The pass driver behind ststhip_app_run and stencil::hip::StencilUpdate: splits n_iterations into
 * launches of the compiled blocking depths, ping-pongs between `dst` and pooled scratch planes so
 * that the last pass lands in `dst` (`src` is never written), and -- for tall grids -- advances
 * two row strips on separate streams, so that the tail of one launch overlaps with the next
 * launches: strips whose common boundary moves up by a launch's ghost rows from pass to pass
 * (ststhip_options::skewed_strips; the upper strip then never waits for the lower one), or fixed
 * strips coupled through boundary bands.  `sweep` performs one launch (for C++ transition
 * functions it is instantiated in the user's translation unit). */
typedef int (*ststhip_sweep_fn)(void *ctx, const ststhip_domain *dom, const void *const *src,
                                void *const *dst, uint64_t out_row_begin, uint64_t out_row_end,
                                uint64_t iteration, uint32_t n_generations, ststhip_stream stream);
typedef struct {
    uint32_t n_planes;
    uint32_t max_generations;           /* deepest blocking `sweep` accepts (powers of two up to it) */
    uint32_t halo_depth_per_generation; /* radius * n_subiterations */
    uint32_t strip_width;               /* columns one wave produces at max_generations (0 = unknown) */
    uint64_t plane_elem_size[16];
    /* Time-dependent values (0 / NULL: the sweep callback provides them per launch).  The driver builds ONE device
     * table per call -- element i = value of generation iteration_offset + i -- either by calling fill_tdv (host
     * evaluation, once per generation as the reference's backends do, cuda/StencilUpdate.hpp:224) and uploading
     * it, or by taking `tdv_device_table` (n_iterations values the caller has already computed on the device). */
    uint64_t tdv_size;
    void (*fill_tdv)(void *ctx, uint64_t iteration_offset, uint64_t n_iterations, void *values);
    const void *tdv_device_table;
    /* Depth by measurement (ABI 5; 0 / 0: none).  The deepest compiled depth is not the fastest for every function and
     * grid: what a transition function costs per cell is opaque to the rule that sizes the pipeline from the cell (the
     * same five-point Jacobi source is nine operations per cell compiled with -ffp-contract=off and five with fused
     * multiply-adds: the first is fastest at 8 generations per launch, the second at 16), and a small grid pays more
     * for deep halos than a large one.  `alt_generations` names a second depth `sweep` accepts (a repeated halving of
     * max_generations: any other value is refused with STSTHIP_ERR_INVALID) and is the depth of every launch nobody has
     * measured.  Where alt_generations does not divide max_generations (18 -> 9 -> 4), or both are odd (27 and 3),
     * nothing is measured: every launch runs at alt_generations.  Otherwise, on the first call for a grid shape that is
     * long enough (>= 6 launches of max_generations) the pass driver times two launches of max_generations against the
     * same generations at alt_generations -- these are the call's own first passes, no work is repeated --, keeps the
     * faster for the rest of the call and, per (tune_key, height, width), for the process
     * (ststhip_tuned_depth reads the choice).  Results do not depend on it.  `tune_key` identifies the kernel family
     * (e.g. the address of the launch callback). */
    uint32_t alt_generations;
    uint32_t reserved;
    uint64_t tune_key;
} ststhip_sweep_desc;
int ststhip_run_passes(ststhip_sweep_fn sweep, void *ctx, const ststhip_sweep_desc *desc,
                       const ststhip_domain *dom, const void *const *src, void *const *dst,
                       uint64_t iteration_offset, uint64_t n_iterations, int blocking, int profiling,
                       ststhip_stream stream, ststhip_run_info *info);
/* A source that is still on its way (ABI 6).  A grid's first update pays for its upload: 1 GiB takes 18.7 ms over PCIe,
 * a quarter of a 1000-generation run of the Jacobi example, and in front of the first pass the chip idles for all of
 * it.  A host that uploads in ROW BLOCKS (in order, first rows first) names them here for the calling thread's NEXT
 * ststhip_run_passes / ststhip_app_run call: rows [blocks[i-1].row_end, blocks[i].row_end) of every source plane are in
 * HBM once event blocks[i].ready has completed (the last row_end >= the grid's height; the call consumes the list
 * whatever it returns, also when it refuses its arguments before any work: a later call never sees it).  The driver
 * then starts on what has arrived: it runs its first passes as row tiles skewed in
 * time -- pass p of the rows above block boundary b reaches g*(p+1) rows less far down than the boundary, g = ghost
 * rows of one launch, so that every tile depends only on tiles of rows that arrived earlier --, as many passes deep
 * as it takes to keep the chip busy between two arrivals (measured per call: the first tile column is timed against
 * the gap between the arrival events), completes those passes over the whole grid when the last block is there and
 * continues with whole-grid passes.  The targets alternate exactly as without the list, the result is the same bit for
 * bit.  The host thread waits for the arrival events inside the call (also with blocking = 0).  `stream` must NOT be
 * made to wait for the upload by the caller; when the driver cannot use the list (profiling runs, grids of few rows per
 * block, options.stream_upload = 0) it makes `stream` wait for every block itself. */
typedef struct {
    uint64_t row_end;
    ststhip_event ready;
} ststhip_source_block;
int ststhip_set_source_arrival(const ststhip_source_block *blocks, uint32_t n_blocks);
/* The rule for such an upload: into how many row blocks (1 = do not split) a host should divide `rows` rows of
 * `row_bytes` bytes (all planes together), and the streams the runtime keeps for it: `copies` for the transfers
 * (ordered against nothing else) and `work` for kernels a host runs per block behind its copy (the scatter into
 * per-field planes; an event per block carries the order: a kernel queued on the copies' own stream holds up the next
 * transfer until it has found room on the chip).  Both are streams of the pass driver that idle while a source
 * arrives -- its tiles run on the caller's stream and the driver's side stream. */
int ststhip_suggest_upload_blocks(uint64_t rows, uint64_t row_bytes, uint32_t *n_blocks);
int ststhip_upload_streams(ststhip_stream *copies, ststhip_stream *work);

/* The depth the pass driver has measured to be the faster one for (tune_key, height, width) in this process; 0 = not
 * measured yet. */
int ststhip_tuned_depth(uint64_t tune_key, uint64_t height, uint64_t width, uint32_t *depth);
/* The same for a precompiled transition function (its kernel family's key is internal to the registry). */
int ststhip_app_tuned_depth(const char *app, uint64_t height, uint64_t width, uint32_t *depth);

/* Parameter blocks of the precompiled transition functions (plain data, host side). */
typedef struct {
    float coef[9]; /* as many as the variant takes; Jacobi9General: coef[r*3+c] */
} ststhip_jacobi_params;
typedef struct {
    float coef[25]; /* "jacobi25general": dense 5 x 5, radius 2, coef[(dr+2)*5 + (dc+2)] */
} ststhip_jacobi25_params;
typedef struct {
    float Rx_1, Ry_1, Rz_1, Cap_1;
} ststhip_hotspot_params;
typedef struct {
    double Rx_1, Ry_1, Rz_1, Cap_1;
} ststhip_hotspot_params_f64; /* "hotspot_f64" / "hotspot_f64_aos": the same formula in fp64 (an extra) */
typedef struct {
    float dt, t_0, tau, omega;
    uint64_t cutoff_iteration, detect_iteration;
    float source_radius_squared;
    float source_r, source_c, source_distance_bound;
    float double_center_rc;
    uint32_t reserved;
} ststhip_fdtd_params;

/* ------------------------------------------------- multi-GPU ghost exchange */
/* One process per GPU.  The unique id is created on rank 0 and distributed by the host program
 * (torch.distributed / MPI / a file); every rank then joins.  Exchange = grouped ncclSend/ncclRecv
 * with the upper (rank-1) and lower (rank+1) neighbour over the direct xGMI links. */
#define STSTHIP_COMM_ID_BYTES 128
typedef void *ststhip_comm;
int ststhip_comm_unique_id(unsigned char id[STSTHIP_COMM_ID_BYTES]);
int ststhip_comm_create(const unsigned char id[STSTHIP_COMM_ID_BYTES], int rank, int n_ranks,
                        ststhip_comm *comm);
int ststhip_comm_destroy(ststhip_comm comm);
/* The ranks this rank exchanges ghost rows with: `up` holds the rows above its own, `down` the rows below; -1 = no
 * neighbour on that side.  Default after ststhip_comm_create: a chain, rank-1 above and rank+1 below.  Other wirings
 * are for hosts whose strips are not numbered like their ranks (meshes), for rings -- both sides may name the same
 * rank, the messages are posted so that its upper rows arrive below and its lower rows above -- and for a rank that
 * names ITSELF on both sides: a self send/receive inside one group is legal in RCCL, which lets one GPU run the whole
 * exchange path (dlopen'ed symbols, byte counts, pointer arithmetic, stream order) without a second device. */
int ststhip_comm_set_neighbours(ststhip_comm comm, int up, int down);
int ststhip_comm_neighbours(ststhip_comm comm, int *up, int *down);
/* The same for the ghost COLUMNS of a 2-D block decomposition (ststhip_block_*): `left` holds the columns before this
 * rank's, `right` those after; default -1 / -1.  ststhip_comm_set_mesh wires all four sides for ranks laid out
 * row-major on a mesh_rows x mesh_cols mesh (rank = mesh_row * mesh_cols + mesh_col; mesh_rows * mesh_cols = n_ranks). */
int ststhip_comm_set_column_neighbours(ststhip_comm comm, int left, int right);
int ststhip_comm_set_mesh(ststhip_comm comm, int mesh_rows, int mesh_cols);
/* For every plane p: send `n_rows` rows starting at send_up[p] to the upper neighbour (rank-1 unless set otherwise)
 * and at send_down[p] to the lower one (rank+1), receive into recv_up[p] (from the upper neighbour) and recv_down[p]
 * (from the lower one).  row_bytes[p] = bytes of one row of plane p.  Ranks without a neighbour on a side skip it. */
int ststhip_comm_exchange_rows(ststhip_comm comm, int n_planes, const void *const *send_up,
                               const void *const *send_down, void *const *recv_up,
                               void *const *recv_down, const size_t *row_bytes, size_t n_rows,
                               ststhip_stream stream);

/* For every plane p: send the contiguous block of block_bytes[p] bytes at send_left[p] to the left neighbour and the
 * one at send_right[p] to the right one, receive into recv_left[p] / recv_right[p] (the packed ghost columns of a 2-D
 * block: the block driver packs and unpacks them with small copy kernels). */
int ststhip_comm_exchange_columns(ststhip_comm comm, int n_planes, const void *const *send_left,
                                  const void *const *send_right, void *const *recv_left, void *const *recv_right,
                                  const size_t *block_bytes, ststhip_stream stream);

/* ------------------------------------------------- row-strip driver (one strip per process / GPU)
 * The grid is cut into n_ranks strips of consecutive rows; every process owns one strip on its GPU and keeps it,
 * with ghost rows, in two buffer sets inside the library.  ststhip_strip_advance() is cuda::StencilUpdate::operator()
 * for the whole distributed grid.  Its launches go in groups of m = STSTHIP_EXCHANGE_EVERY (default: 4 for strips
 * of up to 4096 rows, else 2) with ONE exchange of m*T*radius*n_subiterations ghost rows per group (RCCL
 * send/recv with the two neighbours over xGMI on a second stream, no collective): inside a group every launch
 * produces the owned rows widened by the ghost depth the rest of the group still needs; the last launch of a group
 * sweeps the rows next to the neighbours first (one band launch), hands them to the exchange for the next group, and
 * sweeps its interior beside both.  No host code between the launches of a call: a C++ (or any FFI)
 * host calls create / upload / advance / download.  The semantics are those of one StencilUpdate on the whole
 * grid (the reference has no spatial decomposition; role model for "same interface, several devices":
 * StencilStream/monotile/StencilUpdate.hpp:166-227).
 *
 * `comm`: a communicator of exactly the n_ranks strips (ststhip_comm_create), rank r = strip r.  Hosts whose ranks
 * cannot be joined by RCCL (tests: several ranks on one GPU) pass comm = NULL and an `exchange` callback with the
 * contract of ststhip_comm_exchange_rows: it must have filled recv_up / recv_down in stream order of `stream`
 * (a callback that stages through host memory synchronises `stream` itself). */
typedef void *ststhip_strip;
typedef int (*ststhip_exchange_fn)(void *ctx, int n_planes, const void *const *send_up,
                                   const void *const *send_down, void *const *recv_up,
                                   void *const *recv_down, const size_t *row_bytes, size_t n_rows,
                                   ststhip_stream stream);
int ststhip_strip_create(const char *app, const void *tf_params, const void *halo_cell, uint64_t total_rows,
                         uint64_t width, int rank, int n_ranks, ststhip_comm comm, ststhip_exchange_fn exchange,
                         void *exchange_ctx, ststhip_strip *strip);
/* The same strip for a sweep that is not in the registry: the launch callback and description a caller would hand to
 * ststhip_run_passes (the C++ templates instantiate the kernel for a user's transition function in their own
 * translation unit: StencilStream/hip/StripUpdate.hpp).  The buffers are the planes `desc` describes. */
/* The `sweep` callback of a custom strip MUST honour the calling thread's row hole (ststhip_launch_row_hole): the
 * driver sweeps both boundary bands of a strip as one launch over [first owned row, last owned row) with the interior
 * left out as the hole, on a highest-priority stream, while another launch sweeps the interior.  Every launch that
 * goes through the C++ templates' launcher (hip/internal/Sweep.hpp: launch_sweep) does; a callback that ignored the
 * hole would sweep the interior twice (same values, doubled work, no band / exchange overlap). */
int ststhip_strip_create_custom(ststhip_sweep_fn sweep, void *ctx, const ststhip_sweep_desc *desc, uint64_t total_rows,
                                uint64_t width, int rank, int n_ranks, ststhip_comm comm,
                                ststhip_exchange_fn exchange, void *exchange_ctx, ststhip_strip *strip);
int ststhip_strip_destroy(ststhip_strip strip);
/* global rows [row_begin, row_end) this strip owns */
int ststhip_strip_rows(ststhip_strip strip, uint64_t *row_begin, uint64_t *row_end);
/* Device pointer to the first owned row of plane `plane` of the CURRENT buffer set (it changes with every
 * advance) and the bytes per row; rows are dense.  Upload / download with ststhip_memcpy_* on the strip's stream. */
int ststhip_strip_plane(ststhip_strip strip, unsigned plane, void **owned_rows, size_t *row_bytes);
int ststhip_strip_stream(ststhip_strip strip, ststhip_stream *stream);
int ststhip_strip_synchronize(ststhip_strip strip);
/* One ghost exchange outside any timed region (RCCL sets up its channels on first use). */
int ststhip_strip_warm_up(ststhip_strip strip);
/* Advance the whole distributed grid by n_generations generations (every rank calls it with the same arguments). */
int ststhip_strip_advance(ststhip_strip strip, uint64_t iteration_offset, uint64_t n_generations, int blocking);
int ststhip_strip_counters(ststhip_strip strip, uint64_t *n_launches, uint64_t *n_exchanges);

/* ------------------------------------------------- 2-D block decomposition (one block per process / GPU)
 * The grid is cut into mesh_rows x mesh_cols blocks, rank = mesh_row * mesh_cols + mesh_col.  Every process keeps its
 * block with ghost rows AND ghost columns in two buffer sets; the handle is an ststhip_strip: ststhip_strip_advance /
 * _synchronize / _warm_up / _counters / _destroy / _stream work on it.  Per group of launches (STSTHIP_EXCHANGE_EVERY)
 * the ghost cells travel in two phases on the comm stream -- columns first (strided in memory: packed into contiguous
 * staging buffers by a copy kernel, sent, unpacked), then rows over the full buffer width, ghost columns included, which
 * carries the corners --, then every launch of the group sweeps the owned block widened by what the rest of the group
 * still needs.  The minimal form of the reference's tile geometry (StencilStream/tiling/Grid.hpp:305-450): no overlap of
 * exchange and interior (a block's boundary is a frame, not two bands).  mesh_cols = 1 gives the row strips above
 * without their overlap; use ststhip_strip_create for those.  Along every axis that is cut (more than one block) a
 * block must own at least two ghost depths, else STSTHIP_ERR_INVALID; an axis with one block may be as short as the
 * grid is.
 * `comm`: a communicator of the mesh's ranks whose neighbours are wired for the mesh (ststhip_comm_set_mesh), or
 * NULL and the two callbacks (contract of ststhip_comm_exchange_rows; the column callback gets the packed blocks as
 * "one row" of block bytes: send_up = send_left, send_down = send_right, ...). */
int ststhip_block_create(const char *app, const void *tf_params, const void *halo_cell, uint64_t total_rows,
                         uint64_t total_cols, int rank, int mesh_rows, int mesh_cols, ststhip_comm comm,
                         ststhip_exchange_fn exchange_rows, void *exchange_rows_ctx,
                         ststhip_exchange_fn exchange_cols, void *exchange_cols_ctx, ststhip_strip *block);
/* The same for a sweep that is not in the registry (ABI 6): the launch callback + description of ststhip_run_passes, as
 * ststhip_strip_create_custom takes them -- what stencil::hip::BlockUpdate<F> (a user's transition function on a mesh of
 * GPUs) is built on.  The callback must honour the column range of the calling thread's launches
 * (ststhip_launch_columns) and the column geometry of the domain it is handed (col_origin / local_cols); a callback that
 * goes through the C++ templates' launcher (hip/internal/Sweep.hpp: launch_sweep) does. */
int ststhip_block_create_custom(ststhip_sweep_fn sweep, void *ctx, const ststhip_sweep_desc *desc, uint64_t total_rows,
                                uint64_t total_cols, int rank, int mesh_rows, int mesh_cols, ststhip_comm comm,
                                ststhip_exchange_fn exchange_rows, void *exchange_rows_ctx,
                                ststhip_exchange_fn exchange_cols, void *exchange_cols_ctx, ststhip_strip *block);
/* global rows and columns this block owns */
int ststhip_block_geometry(ststhip_strip block, uint64_t *row_begin, uint64_t *row_end, uint64_t *col_begin,
                           uint64_t *col_end);
/* Copy the owned cells of plane `plane` of the current buffer set from / to host memory whose rows are
 * `host_pitch_bytes` apart (2-D copies on the block's stream; both synchronise it before returning). */
int ststhip_block_upload(ststhip_strip block, unsigned plane, const void *host_cells, size_t host_pitch_bytes);
int ststhip_block_download(ststhip_strip block, unsigned plane, void *host_cells, size_t host_pitch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* STSTHIP_H */
