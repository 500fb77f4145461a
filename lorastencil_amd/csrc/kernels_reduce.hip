// kernels_reduce.hip -- reductions over the interior of padded arrays: the statistics of one grid, the difference of two and
// their inner product (lora_plan_stats / lora_plan_diff / lora_plan_dot; host side: reduce.cpp).  Bandwidth-bound: a launch
// reads every cell of its box once.
//
// Layout.  The box (lo / hi per dimension, padded coordinates) is a list of rows; a row is cut into PIECES, the naturally
// aligned units one lane loads at once:
//   KIND_F64X2  16 bytes = 2 fp64 cells   1D arrays and even innermost extents (rows start on 16 bytes)
//   KIND_F64X1   8 bytes = 1 fp64 cell    odd innermost extents (rows are only 8-byte aligned)
//   KIND_BF16X8 16 bytes = 8 bf16 cells   rows are a multiple of 8 cells; the interior starts in the middle of piece 0
// A piece at the edge of a row holds halo cells; they are loaded (they lie inside the padded array, and pieces never cross a
// row) and replaced by a select before any arithmetic, so that no halo value -- a NaN included -- reaches a result.
// The statistics reduce cell by cell; the diff reduces a piece first and tests its sum of squares once (reduce_piece).
// The (row, piece) pairs of the box form one line of `total` pieces.  Workgroup g owns pieces [g * chunk, (g + 1) * chunk);
// its 256 lanes walk it with stride 256, four pieces (bf16: two) in flight per lane.  A lane divides once, for its first piece, and
// then advances (piece, row, plane) by the step's precomputed digits with carries.
//
// Determinism.  The number of workgroups, `chunk` and therefore which lane adds which cell in which order depend on the
// dtype and the box only (reduce.cpp: reduce_geometry).  Lanes reduce in registers, a wave by a fixed xor butterfly,
// the four waves of a workgroup through LDS in wave order; the workgroup's record goes to its own slot of a buffer the plan
// owns (plain vector stores, no atomics, no hand-off inside the launch).  A second launch of one wave folds the slots: lane
// l takes slots l, l + 64, ... in ascending order, then the same butterfly.  Same call, same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.h"
#include "reduce_device.h"

namespace lora {

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
// A piece as loaded (raw) and cell j of it as a double (bf16 -> fp64 is exact: a bf16 is the upper half of an fp32).
template <int KIND>
struct PieceOf;
template <>
struct PieceOf<KIND_F64X2> {
    static constexpr int cells = 2;
    typedef f64x2 Raw;
    __device__ static __forceinline__ Raw load(const void *base, long off) {
        return *reinterpret_cast<const f64x2 *>(static_cast<const double *>(base) + off);
    }
    __device__ static __forceinline__ double get(const Raw &r, int j) { return r[j]; }
    __device__ static __forceinline__ double get_or_zero(const Raw &r, int j, bool keep) { return keep ? r[j] : 0.0; }
};
template <>
struct PieceOf<KIND_F64X1> {
    static constexpr int cells = 1;
    typedef double Raw;
    __device__ static __forceinline__ Raw load(const void *base, long off) { return static_cast<const double *>(base)[off]; }
    __device__ static __forceinline__ double get(const Raw &r, int) { return r; }
    __device__ static __forceinline__ double get_or_zero(const Raw &r, int, bool keep) { return keep ? r : 0.0; }
};
template <>
struct PieceOf<KIND_BF16X8> {
    static constexpr int cells = 8;
    typedef u32x4 Raw;
    __device__ static __forceinline__ Raw load(const void *base, long off) {
        return *reinterpret_cast<const u32x4 *>(static_cast<const unsigned short *>(base) + off);
    }
    __device__ static __forceinline__ double get(const Raw &r, int j) {  // two cells per word, the low half first
        const unsigned int w = r[j >> 1];
        return (double) __uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    __device__ static __forceinline__ double get_or_zero(const Raw &r, int j, bool keep) {  // (the select on 32 bits)
        const unsigned int w = r[j >> 1];
        return (double) __uint_as_float(keep ? ((j & 1) ? (w & 0xffff0000u) : (w << 16)) : 0u);
    }
};

// ---- the two reductions: per-lane state, one cell, merge of two states ------------------------------------------------
struct StatsAcc {
    double mn, mx, sum, sq;
    long long nf;
    __device__ __forceinline__ void init() {
        mn = __longlong_as_double(0x7ff0000000000000LL);
        mx = -mn;
        sum = sq = 0.0;
        nf = 0;
    }
    __device__ __forceinline__ void cell(bool valid, double x, double, long) {
        const bool ok = valid && finite64(x);
        nf += (valid && !ok) ? 1 : 0;
        const double y = ok ? x : 0.0;
        sum += y;
        sq += y * y;
        mn = (ok && x < mn) ? x : mn;
        mx = (ok && x > mx) ? x : mx;
    }
    __device__ __forceinline__ void merge(double omn, double omx, double osum, double osq, long long onf) {
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        sum += osum;
        sq += osq;
        nf += onf;
    }
    __device__ __forceinline__ void merge_lane(int m) {  // with the state of lane ^ m
        merge(__shfl_xor(mn, m), __shfl_xor(mx, m), __shfl_xor(sum, m), __shfl_xor(sq, m), __shfl_xor(nf, m));
    }
    __device__ __forceinline__ void merge_record(const ReduceRecord &r) { merge(r.f[0], r.f[1], r.f[2], r.f[3], r.i[0]); }
    __device__ __forceinline__ void to(ReduceRecord &r) const {
        r.f[0] = mn;
        r.f[1] = mx;
        r.f[2] = sum;
        r.f[3] = sq;
        r.i[0] = nf;
        r.i[1] = 0;
    }
};

template <int KIND>
__device__ __forceinline__ void reduce_piece(StatsAcc &acc, const ReduceArgs &a, const Cursor &c, const typename PieceOf<KIND>::Raw &ra,
                                             const typename PieceOf<KIND>::Raw &) {
    typedef PieceOf<KIND> P;
    const int col0 = (a.q0 + c.q) * P::cells;
#pragma unroll
    for (int j = 0; j < P::cells; ++j) {
        const int col = col0 + j;
        acc.cell(col >= a.col_lo && col < a.col_hi, P::get(ra, j), 0.0, c.off + j);
    }
}

// A piece of two grids.  Halo cells count as a = b = 0, which adds nothing to any result of a piece that has an interior
// cell -- every piece has.  The sum of the squares tells whether every difference was finite (and no square overflowed):
// then the piece's three values go in as they are; else the piece is done again cell by cell.
template <int KIND>
__device__ __forceinline__ void reduce_piece(DiffAcc &acc, const ReduceArgs &a, const Cursor &c, const typename PieceOf<KIND>::Raw &ra,
                                             const typename PieceOf<KIND>::Raw &rb) {
    typedef PieceOf<KIND> P;
    // (unsigned: cells left of the box wrap to huge values)
    const unsigned first = (unsigned) ((a.q0 + c.q) * P::cells - a.col_lo), width = (unsigned) (a.col_hi - a.col_lo);
    double s = 0.0, pm = 0.0, am = 0.0;
#pragma unroll
    for (int j = 0; j < P::cells; ++j) {
        const bool valid = first + j < width;
        const double x = P::get_or_zero(ra, j, valid), d = x - P::get_or_zero(rb, j, valid);  // bf16 cells are exact in fp64: one rounding
        s = fma(d, d, s);
        pm = fmax(pm, fabs(d));
        am = fmax(am, fabs(x));
    }
    if (!finite64(s)) {
        s = am = 0.0;
        pm = -1.0;
#pragma unroll
        for (int j = 0; j < P::cells; ++j) {
            const bool valid = first + j < width;
            const double x = P::get(ra, j), d = x - P::get(rb, j);
            const bool ok = valid && finite64(d);
            acc.nf += (valid && !ok) ? 1 : 0;
            s += ok ? d * d : 0.0;
            am = (ok && fabs(x) > am) ? fabs(x) : am;  // d finite => a finite
            pm = (ok && fabs(d) > pm) ? fabs(d) : pm;
        }
    }
    acc.sq += s;
    acc.amax = am > acc.amax ? am : acc.amax;
    const bool take = pm > acc.mx;
    acc.mx = take ? pm : acc.mx;
    acc.idx = take ? (long long) c.off : acc.idx;
}

// A piece of two grids as products a * b (lora_plan_dot).  Halo cells count as a = b = 0.  The sum of the magnitudes tells
// whether every product was finite (and no sum overflowed); else the piece is done again cell by cell.
template <int KIND>
__device__ __forceinline__ void reduce_piece(DotAcc &acc, const ReduceArgs &a, const Cursor &c, const typename PieceOf<KIND>::Raw &ra,
                                             const typename PieceOf<KIND>::Raw &rb) {
    typedef PieceOf<KIND> P;
    const unsigned first = (unsigned) ((a.q0 + c.q) * P::cells - a.col_lo), width = (unsigned) (a.col_hi - a.col_lo);
    double x[P::cells], y[P::cells];
    bool valid[P::cells];
#pragma unroll
    for (int j = 0; j < P::cells; ++j) {
        valid[j] = first + j < width;
        x[j] = P::get_or_zero(ra, j, valid[j]);
        y[j] = P::get_or_zero(rb, j, valid[j]);
    }
    acc.cells<P::cells>(x, y, valid);
}

// (four workgroups per CU, so that the kReduceMaxGroups of a big launch are all resident: 128 registers per lane at most)
template <typename ACC, int KIND, bool DIFF>
__global__ __launch_bounds__(kThreads, 4) void reduce_kernel(const void *__restrict__ pa, const void *__restrict__ pb, const ReduceArgs a,
                                                          ReduceRecord *__restrict__ partial) {
    typedef PieceOf<KIND> P;
    typedef typename P::Raw Raw;
    // pieces a lane loads before it reduces them (eight cells a piece cost bf16 the registers of two)
    constexpr int kInFlight = KIND == KIND_BF16X8 ? 2 : 4;
    ACC acc;
    acc.init();
    const long first = (long) blockIdx.x * a.chunk;
    const long end = first + a.chunk < a.total ? first + a.chunk : a.total;
    long i = first + threadIdx.x;
    Cursor c;
    {
        const long row = i / a.ppr;
        const long i0 = row / a.e1;
        c.q = (int) (i - row * a.ppr);
        c.i1 = (int) (row - i0 * a.e1);
        c.off = a.off0 + i0 * a.plane_stride + c.i1 * a.row_stride + (long) c.q * P::cells;
    }
    // several pieces in flight per lane while as many whole strides remain ...
    for (; i + (kInFlight - 1) * kThreads < end; i += kInFlight * kThreads) {
        Cursor cs[kInFlight];
        Raw ra[kInFlight], rb[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            cs[u] = c;
            c.advance(a);
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            ra[u] = P::load(pa, cs[u].off);
            rb[u] = DIFF ? P::load(pb, cs[u].off) : ra[u];
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) reduce_piece<KIND>(acc, a, cs[u], ra[u], rb[u]);
    }
    // ... then one at a time
    for (; i < end; i += kThreads) {
        const Raw ra = P::load(pa, c.off);
        const Raw rb = DIFF ? P::load(pb, c.off) : ra;
        reduce_piece<KIND>(acc, a, c, ra, rb);
        c.advance(a);
    }

    wave_reduce(acc);
    __shared__ ReduceRecord sh[kThreads / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) acc.to(sh[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) acc.merge_record(sh[w]);
        ReduceRecord r;
        acc.to(r);
        partial[blockIdx.x] = r;
    }
}

// the cell of the maximum inside its piece: the first interior one whose difference is finite and as large
template <int KIND>
__device__ __forceinline__ void resolve_cell(DiffAcc &acc, const ReduceArgs &a, const void *pa, const void *pb) {
    typedef PieceOf<KIND> P;
    if (acc.mx < 0.0) return;  // no finite difference anywhere
    const typename P::Raw ra = P::load(pa, acc.idx), rb = P::load(pb, acc.idx);
    const unsigned first = (unsigned) (int) (acc.idx % a.row_stride - a.col_lo), width = (unsigned) (a.col_hi - a.col_lo);
    int found = 0;
#pragma unroll
    for (int j = P::cells - 1; j >= 0; --j) {
        const double d = P::get(ra, j) - P::get(rb, j);
        found = (first + j < width && finite64(d) && fabs(d) == acc.mx) ? j : found;
    }
    acc.idx += found;
}
__device__ __forceinline__ void resolve(StatsAcc &, const ReduceArgs &, int, const void *, const void *) {}
__device__ __forceinline__ void resolve(DotAcc &, const ReduceArgs &, int, const void *, const void *) {}
__device__ __forceinline__ void resolve(DiffAcc &acc, const ReduceArgs &a, int kind, const void *pa, const void *pb) {
    if (kind == KIND_F64X2)
        resolve_cell<KIND_F64X2>(acc, a, pa, pb);
    else if (kind == KIND_F64X1)
        resolve_cell<KIND_F64X1>(acc, a, pa, pb);
    else if (kind == KIND_BF16X8)
        resolve_cell<KIND_BF16X8>(acc, a, pa, pb);
    // (KIND_CELL: the records carry the cell's own index -- grid `a` of a fused residual is not in memory to be re-read)
}


// the second launch: one wave folds the `groups` records into record `kReduceMaxGroups` of the same buffer
template <typename ACC>
__global__ __launch_bounds__(64) void combine_kernel(ReduceRecord *__restrict__ partial, int groups, const ReduceArgs a, int kind,
                                                     const void *__restrict__ pa, const void *__restrict__ pb) {
    ACC acc;
    acc.init();
    for (int g = threadIdx.x; g < groups; g += 64) acc.merge_record(partial[g]);
    wave_reduce(acc);
    if (threadIdx.x == 0) {
        resolve(acc, a, kind, pa, pb);
        ReduceRecord r;
        acc.to(r);
        partial[kReduceMaxGroups] = r;
    }
}

template <typename ACC, bool DIFF>
hipError_t launch(const ReduceArgs &a, int kind, int groups, const void *pa, const void *pb, ReduceRecord *partial, hipStream_t s) {
    if (kind == KIND_F64X2)
        hipLaunchKernelGGL((reduce_kernel<ACC, KIND_F64X2, DIFF>), dim3(groups), dim3(kThreads), 0, s, pa, pb, a, partial);
    else if (kind == KIND_F64X1)
        hipLaunchKernelGGL((reduce_kernel<ACC, KIND_F64X1, DIFF>), dim3(groups), dim3(kThreads), 0, s, pa, pb, a, partial);
    else
        hipLaunchKernelGGL((reduce_kernel<ACC, KIND_BF16X8, DIFF>), dim3(groups), dim3(kThreads), 0, s, pa, pb, a, partial);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(combine_kernel<ACC>, dim3(1), dim3(64), 0, s, partial, groups, a, kind, pa, pb);
    return hipGetLastError();
}

}  // namespace

int reduce_threads() { return kThreads; }

hipError_t launch_reduce_stats(const ReduceArgs &a, int kind, int groups, const void *buf, ReduceRecord *partial, hipStream_t s) {
    return launch<StatsAcc, false>(a, kind, groups, buf, nullptr, partial, s);
}

hipError_t launch_reduce_diff(const ReduceArgs &a, int kind, int groups, const void *buf_a, const void *buf_b, ReduceRecord *partial,
                              hipStream_t s) {
    return launch<DiffAcc, true>(a, kind, groups, buf_a, buf_b, partial, s);
}

// sum of a * b over the box (lora_plan_dot; a == b allowed: the grid is then loaded twice)
hipError_t launch_reduce_dot(const ReduceArgs &a, int kind, int groups, const void *buf_a, const void *buf_b, ReduceRecord *partial,
                             hipStream_t s) {
    return launch<DotAcc, true>(a, kind, groups, buf_a, buf_b, partial, s);
}

// the fold alone, over difference records that carry cell indices (kernels_residual.hip)
hipError_t launch_reduce_fold_cells(int groups, ReduceRecord *partial, hipStream_t s) {
    hipLaunchKernelGGL(combine_kernel<DiffAcc>, dim3(1), dim3(64), 0, s, partial, groups, ReduceArgs{}, (int) KIND_CELL,
                       (const void *) nullptr, (const void *) nullptr);
    return hipGetLastError();
}

}  // namespace lora
