// ststhip_grid_copy / _fill / _download / _upload (include/ststhip.h): rectangles of a grid, or of one member of its
// cells, moved where the cells are.
//
// Three kernels, all built the way norms.hip walks a rectangle: a workgroup owns row segments -- segment blockIdx.x of
// rows blockIdx.y, + gridDim.y, ... of the rectangle --, consecutive lanes take consecutive elements of one row, the
// address arithmetic per row is wave-uniform (64-bit) and a lane adds a 32-bit offset (the validation keeps a row's
// byte extent below 2^31).  No division per element, no atomics, no LDS, no scratch; the number of workgroups follows
// from the rectangle alone, capped by a constant.
//
//   copy_rows_kernel     both sides dense within a row (stride == elem_size, column step 1): a row is a run of bytes.
//                        Per row the widest access that both addresses allow (16, 8, 4, 2 or 1 bytes, from how the two
//                        sit relative to each other), an unaligned head and tail peeled off as bytes.
//   copy_strided_kernel  members of cells, steps, odd element sizes: one element per lane, as elem_size / sizeof(W)
//                        accesses of the widest unit W that bases, strides, row distances and the size all allow:
//                        one native 1/2/4/8/16-byte access where that is the element, else words, else bytes.
//   fill_strided_kernel  the same walk with the value from the kernel's arguments.
#include "ststhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

namespace ststhip_detail {
int fail(int status, const char *message); // runtime.hip
}

namespace {

using u64 = unsigned long long;

constexpr unsigned region_threads = 256;
// A row segment of the dense kernel: four 16-byte accesses per lane.
constexpr unsigned region_segment_bytes = 4 * 16 * region_threads;
// A row segment of the strided kernels: four elements per lane.
constexpr unsigned region_segment_cells = 4 * region_threads;
// At most this many workgroups per launch (or one per segment of a row, if a row alone has more): 8 per CU of a
// 256-CU chip, as the norms.
constexpr unsigned region_block_cap = 2048;
constexpr unsigned region_max_elem = 128;

typedef unsigned Word16 __attribute__((ext_vector_type(4)));

// One entry as the kernels see it: dst / src are the first element of the rectangle.
struct RowJob {
    unsigned char *dst;
    const unsigned char *src;
    u64 dst_row_bytes, src_row_bytes; // bytes between two rows of the rectangle (the source's row step included)
    unsigned n_rows;
    unsigned row_len;            // dense: bytes of a row of the rectangle; strided: its elements
    unsigned dst_step, src_step; // strided: bytes between two elements of a row (the source's column step included)
    unsigned elem_size;
};

struct FillJob {
    unsigned char *dst;
    u64 dst_row_bytes;
    unsigned n_rows, row_len, dst_step, elem_size;
    alignas(16) unsigned char value[region_max_elem];
};

// n units of sizeof(W) bytes from s to d, both aligned to it, by the whole workgroup: the four loads of a lane are
// requested before the first store.
template <typename W> __device__ inline void copy_units(unsigned char *d, const unsigned char *s, unsigned n) {
    for (unsigned base = 0; base < n; base += 4 * region_threads) {
        W v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned i = base + threadIdx.x + k * region_threads;
            if (i < n)
                v[k] = reinterpret_cast<const W *>(s)[i];
        }
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned i = base + threadIdx.x + k * region_threads;
            if (i < n)
                reinterpret_cast<W *>(d)[i] = v[k];
        }
    }
}

__global__ void __launch_bounds__(region_threads) copy_rows_kernel(RowJob j) {
    const unsigned seg_begin = blockIdx.x * region_segment_bytes; // < row_len < 2^31
    const unsigned rest = j.row_len - seg_begin;
    const unsigned len = rest < region_segment_bytes ? rest : region_segment_bytes;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + seg_begin);
        const unsigned char *s = j.src + (u64(r) * j.src_row_bytes + seg_begin);
        // the widest access both sides allow: the lowest set bit of their distance, 16 at the most
        const unsigned apart = (unsigned(reinterpret_cast<std::uintptr_t>(d)) - unsigned(reinterpret_cast<std::uintptr_t>(s))) | 16u;
        const unsigned w = apart & (0u - apart);
        unsigned head = (0u - unsigned(reinterpret_cast<std::uintptr_t>(d))) & (w - 1u);
        head = head < len ? head : len;
        const unsigned n_units = (len - head) / w;
        const unsigned tail_begin = head + n_units * w;
        const unsigned n_edge = head + (len - tail_begin); // < 32
        switch (w) {
        case 16: copy_units<Word16>(d + head, s + head, n_units); break;
        case 8: copy_units<std::uint64_t>(d + head, s + head, n_units); break;
        case 4: copy_units<std::uint32_t>(d + head, s + head, n_units); break;
        case 2: copy_units<std::uint16_t>(d + head, s + head, n_units); break;
        default: copy_units<std::uint8_t>(d + head, s + head, n_units);
        }
        if (threadIdx.x < n_edge) {
            const unsigned e = threadIdx.x < head ? threadIdx.x : tail_begin + (threadIdx.x - head);
            d[e] = s[e];
        }
    }
}

template <typename W> __global__ void __launch_bounds__(region_threads) copy_strided_kernel(RowJob j) {
    const unsigned n_units = j.elem_size / unsigned(sizeof(W));
    const unsigned seg_begin = blockIdx.x * region_segment_cells; // < row_len < 2^31
    const unsigned rest = j.row_len - seg_begin;
    const unsigned len = rest < region_segment_cells ? rest : region_segment_cells;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        const unsigned char *s = j.src + (u64(r) * j.src_row_bytes + u64(seg_begin) * j.src_step);
        if (n_units == 1) {
            W v[4];
#pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const unsigned c = threadIdx.x + k * region_threads;
                if (c < len)
                    v[k] = *reinterpret_cast<const W *>(s + c * j.src_step);
            }
#pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const unsigned c = threadIdx.x + k * region_threads;
                if (c < len)
                    *reinterpret_cast<W *>(d + c * j.dst_step) = v[k];
            }
        } else {
            for (unsigned c = threadIdx.x; c < len; c += region_threads) {
                const W *from = reinterpret_cast<const W *>(s + c * j.src_step);
                W *to = reinterpret_cast<W *>(d + c * j.dst_step);
                for (unsigned u = 0; u < n_units; u++)
                    to[u] = from[u];
            }
        }
    }
}

template <typename W> __global__ void __launch_bounds__(region_threads) fill_strided_kernel(FillJob j) {
    const unsigned n_units = j.elem_size / unsigned(sizeof(W));
    const unsigned seg_begin = blockIdx.x * region_segment_cells;
    const unsigned rest = j.row_len - seg_begin;
    const unsigned len = rest < region_segment_cells ? rest : region_segment_cells;
    const W *value = reinterpret_cast<const W *>(j.value);
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        for (unsigned u = 0; u < n_units; u++) {
            const W v = value[u]; // the same for every lane
            for (unsigned c = threadIdx.x; c < len; c += region_threads)
                reinterpret_cast<W *>(d + c * j.dst_step)[u] = v;
        }
    }
}

// ------------------------------------------------------------------ host side
static int invalid(const char *what) {
    const std::string msg = std::string("grid region: ") + what;
    return ststhip_detail::fail(STSTHIP_ERR_INVALID, msg.c_str());
}

static int hip_failed(hipError_t err, const char *what) {
    const std::string msg = std::string(what) + ": " + hipGetErrorString(err);
    return ststhip_detail::fail(STSTHIP_ERR_HIP, msg.c_str());
}

// What does not depend on the rectangle.  0 = fine.
static int check_view(ststhip_grid_view const &v, unsigned elem_size) {
    if (v.stride == 0)
        return invalid("stride 0");
    if (elem_size > v.stride)
        return invalid("elem_size above the stride");
    if (v.pitch < v.width)
        return invalid("pitch < width");
    // every byte offset formed, (r * pitch + c) * stride with r < height and c < width <= pitch, fits in 63 bits
    u64 row_bytes = 0, grid_bytes = 0;
    if (__builtin_mul_overflow(u64(v.pitch), u64(v.stride), &row_bytes) ||
        __builtin_mul_overflow(row_bytes, u64(v.height) + 1, &grid_bytes) || v.height + 1 == 0 || grid_bytes >> 63 != 0)
        return invalid("extents, pitch and stride describe more than 2^63 bytes");
    return 0;
}

// The cells first, first + step, ..., n of them, lie inside [0, extent).  n >= 1.
static bool inside(u64 first, u64 n, u64 step, u64 extent) {
    u64 reach = 0;
    return first < extent && !__builtin_mul_overflow(n - 1, step, &reach) && reach <= extent - 1 - first;
}

static int check_size(unsigned elem_size, u64 n_rows, u64 n_cols) {
    if (elem_size < 1 || elem_size > region_max_elem)
        return invalid("elem_size outside 1..128");
    if (n_rows >> 31 != 0 || n_cols >> 31 != 0)
        return invalid("n_rows or n_cols of 2^31 or more");
    return 0;
}

// A rectangle's row in a view: n_cols * step * stride bytes, below 2^31.
static bool row_fits(u64 n_cols, u64 step, u64 stride) {
    u64 a = 0, b = 0;
    return !__builtin_mul_overflow(n_cols, step, &a) && !__builtin_mul_overflow(a, stride, &b) && b >> 31 == 0;
}

enum class Host { none, dst, src };

// One copy entry, validated and reduced to what a kernel needs.  `empty`: nothing to move.
struct Plan {
    bool empty = true;
    RowJob job{};
};

static int plan_copy(ststhip_grid_copy_desc const &c, Host host, Plan &plan) {
    if (int rc = check_size(c.elem_size, c.n_rows, c.n_cols))
        return rc;
    if (int rc = check_view(c.dst, c.elem_size))
        return rc;
    if (int rc = check_view(c.src, c.elem_size))
        return rc;
    if (c.src_row_step == 0 || c.src_col_step == 0)
        return invalid("a step of 0");
    if (host == Host::dst && c.dst.stride != c.elem_size)
        return invalid("the host side of a download must be dense within a row (dst.stride == elem_size)");
    if (host == Host::src && (c.src.stride != c.elem_size || c.src_row_step != 1 || c.src_col_step != 1))
        return invalid("the host side of an upload must be dense within a row (src.stride == elem_size, steps 1)");
    plan.empty = c.n_rows == 0 || c.n_cols == 0;
    if (plan.empty)
        return 0;
    if (!c.dst.base || !c.src.base)
        return invalid("null base with a non-empty rectangle");
    if (!inside(c.dst_row, c.n_rows, 1, c.dst.height) || !inside(c.dst_col, c.n_cols, 1, c.dst.width))
        return invalid("the destination rectangle does not lie inside its view");
    if (!inside(c.src_row, c.n_rows, c.src_row_step, c.src.height) || !inside(c.src_col, c.n_cols, c.src_col_step, c.src.width))
        return invalid("the source rectangle does not lie inside its view");
    if (!row_fits(c.n_cols, 1, c.dst.stride) || !row_fits(c.n_cols, c.src_col_step, c.src.stride))
        return invalid("a row of the rectangle spans 2^31 bytes or more");

    RowJob &j = plan.job;
    // (all products below are bounded by the views' byte sizes, which check_view has found to fit)
    j.dst = static_cast<unsigned char *>(c.dst.base) + (c.dst_row * c.dst.pitch + c.dst_col) * c.dst.stride;
    j.src = static_cast<const unsigned char *>(c.src.base) + (c.src_row * c.src.pitch + c.src_col) * c.src.stride;
    j.dst_row_bytes = c.dst.pitch * c.dst.stride;
    j.src_row_bytes = c.src.pitch * c.src.stride * c.src_row_step; // (used with more than one row only)
    j.n_rows = unsigned(c.n_rows);
    j.row_len = unsigned(c.n_cols);
    j.dst_step = unsigned(c.dst.stride);
    j.src_step = unsigned(c.src.stride * c.src_col_step);
    j.elem_size = c.elem_size;
    if (c.n_cols == 1) { // (a single column: the strides may be anything, the steps are never used)
        j.dst_step = j.src_step = c.elem_size;
    }
    if (c.n_rows == 1)
        j.dst_row_bytes = j.src_row_bytes = 0;

    if (host == Host::none) {
        // overlap: the byte spans first element .. last byte of the last element
        const std::uintptr_t d0 = reinterpret_cast<std::uintptr_t>(j.dst), s0 = reinterpret_cast<std::uintptr_t>(j.src);
        const u64 d_span = (c.n_rows - 1) * c.dst.pitch * c.dst.stride + (c.n_cols - 1) * c.dst.stride + c.elem_size;
        const u64 s_span = (c.n_rows - 1) * c.src.pitch * c.src.stride * c.src_row_step +
                           (c.n_cols - 1) * c.src.stride * c.src_col_step + c.elem_size;
        if (d0 < s0 + s_span && s0 < d0 + d_span) {
            const u64 apart = d0 > s0 ? d0 - s0 : s0 - d0;
            const bool members = c.dst.stride == c.src.stride && c.dst.pitch == c.src.pitch && c.src_row_step == 1 &&
                                 c.src_col_step == 1 && apart >= c.elem_size && apart < c.src.stride &&
                                 apart + c.elem_size <= c.src.stride;
            if (!members)
                return invalid("source and destination overlap (only a member copied to another member of the same "
                               "cells may share memory)");
        }
    }
    return 0;
}

// Workgroups of a launch over n_rows rows of n_segments segments.
static dim3 plan_blocks(u64 n_segments, u64 n_rows) {
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, region_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

// The widest unit (16, 8, 4, 2, 1) that divides everything in `bits`.
static unsigned unit_of(u64 bits) {
    const u64 b = bits | 16u;
    return unsigned(b & (0 - b));
}

static hipError_t launch_copy(RowJob j, hipStream_t s) {
    if (j.dst_step == j.elem_size && j.src_step == j.elem_size) {
        j.row_len *= j.elem_size; // < 2^31: the row's byte extent
        const dim3 grid = plan_blocks((u64(j.row_len) + region_segment_bytes - 1) / region_segment_bytes, j.n_rows);
        hipLaunchKernelGGL(copy_rows_kernel, grid, dim3(region_threads), 0, s, j);
        return hipGetLastError();
    }
    const unsigned unit = unit_of(reinterpret_cast<std::uintptr_t>(j.dst) | reinterpret_cast<std::uintptr_t>(j.src) |
                                  j.dst_row_bytes | j.src_row_bytes | j.dst_step | j.src_step | j.elem_size);
    const dim3 grid = plan_blocks((u64(j.row_len) + region_segment_cells - 1) / region_segment_cells, j.n_rows);
    switch (unit) {
    case 16: hipLaunchKernelGGL(copy_strided_kernel<Word16>, grid, dim3(region_threads), 0, s, j); break;
    case 8: hipLaunchKernelGGL(copy_strided_kernel<std::uint64_t>, grid, dim3(region_threads), 0, s, j); break;
    case 4: hipLaunchKernelGGL(copy_strided_kernel<std::uint32_t>, grid, dim3(region_threads), 0, s, j); break;
    case 2: hipLaunchKernelGGL(copy_strided_kernel<std::uint16_t>, grid, dim3(region_threads), 0, s, j); break;
    default: hipLaunchKernelGGL(copy_strided_kernel<std::uint8_t>, grid, dim3(region_threads), 0, s, j);
    }
    return hipGetLastError();
}

static hipError_t launch_fill(FillJob const &j, hipStream_t s) {
    const dim3 grid = plan_blocks((u64(j.row_len) + region_segment_cells - 1) / region_segment_cells, j.n_rows);
    const unsigned unit = unit_of(reinterpret_cast<std::uintptr_t>(j.dst) | j.dst_row_bytes | j.dst_step | j.elem_size);
    switch (unit) {
    case 16: hipLaunchKernelGGL(fill_strided_kernel<Word16>, grid, dim3(region_threads), 0, s, j); break;
    case 8: hipLaunchKernelGGL(fill_strided_kernel<std::uint64_t>, grid, dim3(region_threads), 0, s, j); break;
    case 4: hipLaunchKernelGGL(fill_strided_kernel<std::uint32_t>, grid, dim3(region_threads), 0, s, j); break;
    case 2: hipLaunchKernelGGL(fill_strided_kernel<std::uint16_t>, grid, dim3(region_threads), 0, s, j); break;
    default: hipLaunchKernelGGL(fill_strided_kernel<std::uint8_t>, grid, dim3(region_threads), 0, s, j);
    }
    return hipGetLastError();
}

static int resolve_stream(ststhip_stream &stream) {
    if (int rc = ststhip_init(-1))
        return rc;
    if (!stream)
        if (int rc = ststhip_default_stream(&stream))
            return rc;
    return STSTHIP_OK;
}

static int plan_all(int n, const ststhip_grid_copy_desc *copies, Host host, Plan (&plan)[8], bool &any) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!copies)
        return invalid("null argument");
    any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = plan_copy(copies[i], host, plan[i]))
            return rc;
        any = any || !plan[i].empty;
    }
    return 0;
}

// A rectangle between host memory (rows `host_row_bytes` apart) and dense device staging.
static hipError_t copy_host_rows(void *dst, u64 dst_row_bytes, const void *src, u64 src_row_bytes, u64 row_bytes,
                                 u64 n_rows, hipMemcpyKind kind, hipStream_t s) {
    if (n_rows == 1 || (dst_row_bytes == row_bytes && src_row_bytes == row_bytes))
        return hipMemcpyAsync(dst, src, row_bytes * n_rows, kind, s);
    return hipMemcpy2DAsync(dst, dst_row_bytes, src, src_row_bytes, row_bytes, n_rows, kind, s);
}

// download (to_host) and upload: the device side of every entry goes through dense staging from the pool
static int grid_transfer(int n, const ststhip_grid_copy_desc *copies, bool to_host, ststhip_stream stream) {
    Plan plan[8];
    bool any = false;
    if (int rc = plan_all(n, copies, to_host ? Host::dst : Host::src, plan, any))
        return rc;
    if (!any)
        return STSTHIP_OK;
    if (int rc = resolve_stream(stream))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const char *what = to_host ? "ststhip_grid_download" : "ststhip_grid_upload";

    void *staging[8] = {nullptr};
    int rc = STSTHIP_OK;
    hipError_t err = hipSuccess;
    for (int i = 0; i < n && rc == STSTHIP_OK && err == hipSuccess; i++) {
        if (plan[i].empty)
            continue;
        ststhip_grid_copy_desc const &c = copies[i];
        const u64 row_bytes = c.n_cols * c.elem_size;
        rc = ststhip_malloc_async(&staging[i], row_bytes * c.n_rows, stream);
        if (rc != STSTHIP_OK)
            break;
        RowJob j = plan[i].job;
        if (to_host) {
            unsigned char *host = j.dst;
            const u64 host_row_bytes = c.dst.pitch * c.dst.stride;
            j.dst = static_cast<unsigned char *>(staging[i]);
            j.dst_row_bytes = c.n_rows == 1 ? 0 : row_bytes;
            j.dst_step = c.elem_size;
            err = launch_copy(j, s);
            if (err == hipSuccess)
                err = copy_host_rows(host, host_row_bytes, staging[i], row_bytes, row_bytes, c.n_rows, hipMemcpyDeviceToHost, s);
        } else {
            const unsigned char *host = j.src;
            const u64 host_row_bytes = c.src.pitch * c.src.stride;
            j.src = static_cast<const unsigned char *>(staging[i]);
            j.src_row_bytes = c.n_rows == 1 ? 0 : row_bytes;
            j.src_step = c.elem_size;
            err = copy_host_rows(staging[i], row_bytes, host, host_row_bytes, row_bytes, c.n_rows, hipMemcpyHostToDevice, s);
            if (err == hipSuccess)
                err = launch_copy(j, s);
        }
    }
    // the host's memory is read or written by what has been queued, whatever failed after it: wait in every case
    const hipError_t sync = hipStreamSynchronize(s);
    if (err == hipSuccess)
        err = sync;
    for (int i = 0; i < n; i++)
        if (staging[i])
            ststhip_free_async(staging[i], stream);
    if (rc != STSTHIP_OK)
        return rc;
    return err == hipSuccess ? STSTHIP_OK : hip_failed(err, what);
}

} // namespace

extern "C" {

int ststhip_grid_copy(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream) {
    Plan plan[8];
    bool any = false;
    if (int rc = plan_all(n, copies, Host::none, plan, any))
        return rc;
    if (!any)
        return STSTHIP_OK;
    if (int rc = resolve_stream(stream))
        return rc;
    for (int i = 0; i < n; i++) {
        if (plan[i].empty)
            continue;
        const hipError_t err = launch_copy(plan[i].job, static_cast<hipStream_t>(stream));
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_copy");
    }
    return STSTHIP_OK;
}

int ststhip_grid_fill(int n, const ststhip_grid_fill_desc *fills, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!fills)
        return invalid("null argument");
    FillJob job[8];
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        ststhip_grid_fill_desc const &f = fills[i];
        if (int rc = check_size(f.elem_size, f.n_rows, f.n_cols))
            return rc;
        if (int rc = check_view(f.dst, f.elem_size))
            return rc;
        if (!f.value)
            return invalid("null value");
        empty[i] = f.n_rows == 0 || f.n_cols == 0;
        if (empty[i])
            continue;
        if (!f.dst.base)
            return invalid("null base with a non-empty rectangle");
        if (!inside(f.dst_row, f.n_rows, 1, f.dst.height) || !inside(f.dst_col, f.n_cols, 1, f.dst.width))
            return invalid("the destination rectangle does not lie inside its view");
        if (!row_fits(f.n_cols, 1, f.dst.stride))
            return invalid("a row of the rectangle spans 2^31 bytes or more");
        FillJob &j = job[i];
        j.dst = static_cast<unsigned char *>(f.dst.base) + (f.dst_row * f.dst.pitch + f.dst_col) * f.dst.stride;
        j.dst_row_bytes = f.n_rows == 1 ? 0 : f.dst.pitch * f.dst.stride;
        j.n_rows = unsigned(f.n_rows);
        j.row_len = unsigned(f.n_cols);
        j.dst_step = f.n_cols == 1 ? f.elem_size : unsigned(f.dst.stride);
        j.elem_size = f.elem_size;
        std::memset(j.value, 0, sizeof j.value);
        std::memcpy(j.value, f.value, f.elem_size);
        any = true;
    }
    if (!any)
        return STSTHIP_OK;
    if (int rc = resolve_stream(stream))
        return rc;
    for (int i = 0; i < n; i++) {
        if (empty[i])
            continue;
        const hipError_t err = launch_fill(job[i], static_cast<hipStream_t>(stream));
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_fill");
    }
    return STSTHIP_OK;
}

int ststhip_grid_download(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream) {
    return grid_transfer(n, copies, /*to_host=*/true, stream);
}

int ststhip_grid_upload(int n, const ststhip_grid_copy_desc *copies, ststhip_stream stream) {
    return grid_transfer(n, copies, /*to_host=*/false, stream);
}

} // extern "C"
