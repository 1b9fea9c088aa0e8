// What the online statistics kernels share (fg_planestats.hip, fg_planespectra.hip, fg_planebudgets.hip, fg_planetimecorr.hip and,
// for the loads and the order-2 merge, fg_cellstats.hip), each rule written once.  No pragma and no assumption about -ffp-contract:
// every file compiles this header under its own flags.
//
// Ownership and order of the row recorders: one workgroup of 256 threads owns a row (env, y) whose plane [nz, nx] has more than
// WAVE_CELLS cells (the TCF shape 8 x 128 x 64 x 64: 512 rows of 128 x 64 cells), one wave of a four-wave workgroup a smaller one
// (2-D fields: a plane is one x row, so a workgroup takes four y rows).  Every lane adds its cells in ascending order, the lanes
// combine by the xor butterfly of the wave, the waves in ascending order through LDS: a fixed tree, no floating-point atomic
// anywhere, so a row's result depends on nothing but the row's cells and the extents.
//
// Loads: VEC reals by one 16-byte load where nx, every channel pointer and every batch stride allow it (fill decides), one real at
// a time otherwise; the arithmetic does not depend on the form.
//
// Merge: a sample (B) joins the running record (A) by the pairwise update of Pebay et al. 2016 with delta = mean_B - mean_A; at
// order 2 that is the parallel Welford / Schubert-Gertz rule of merge2.  n[env] is read by every row of the env and advanced once
// per call by FG_ROWSTAT_ADVANCE_N.
#pragma once
#include <float.h>

#include <string>
#include <type_traits>

#include "fg_internal.h"

namespace fg_rowstat {

constexpr int VEC = FG_F64 ? 2 : 4;      // reals per 16-byte load
constexpr int WAVE_CELLS = 1024;         // planes up to this many cells are reduced by one wave

// V consecutive reals at p (V == VEC: one 16-byte load) as T = double or fg_real
template <int V, typename T>
__device__ __forceinline__ void load(const fg_real* p, T (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = (T)p[0];
    } else {
#if FG_F64
        const double2 q = *reinterpret_cast<const double2*>(p);
        v[0] = (T)q.x; v[1] = (T)q.y;
#else
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = (T)q.x; v[1] = (T)q.y; v[2] = (T)q.z; v[3] = (T)q.w;
#endif
    }
}

// the sum of v[q] over the lanes of the wave (WAVE) or of the workgroup, left in every lane: xor butterfly, then the four waves in
// ascending order
template <int N, int S, bool WAVE>
__device__ __forceinline__ void reduce(double (&v)[N], double (&s_red)[4][S], int tid) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
    }
    if constexpr (!WAVE) {
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < N; ++q) s_red[tid >> 6][q] = v[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = ((s_red[0][q] + s_red[1][q]) + s_red[2][q]) + s_red[3][q];
        __syncthreads();
    }
}

// Row ownership in a kernel <..., VEC, WAVE> with arguments `a` (rows = batch * ny and the extents nz, ny, nx) and tid = threadIdx.x:
// declares row, b (env), y, and the thread's work items i = t0, t0 + step, ... < items, each VEC consecutive cells in x, nxv of them
// per x row.  In the WAVE form a wave without a row (the last workgroup) returns as a whole; that form has no barrier.  A macro and
// not a type: every struct or function tried for these lines changed the generated code of the kernels (up to two more VGPRs).
#define FG_ROWSTAT_OWN_ROW(a, VEC, WAVE, tid)                                                                  \
    const long long row = WAVE ? (long long)blockIdx.x * 4 + ((tid) >> 6) : (long long)blockIdx.x;             \
    if (WAVE && row >= (a).rows) return;                                                                       \
    const int b = (int)(row / (a).ny), y = (int)(row - (long long)b * (a).ny);                                 \
    const int nxv = (a).nx / VEC, items = (a).nz * nxv;                                                        \
    const int t0 = WAVE ? ((tid) & 63) : (tid), step = WAVE ? 64 : 256

// work item i of a row -> the offset of its first cell from the row's first cell
template <int V>
__device__ __forceinline__ long long item_offset(int i, int nxv, long long zstride) {
    const int z = i / nxv, xv = i - z * nxv;
    return (long long)z * zstride + (long long)xv * V;
}

// the sums of K channels over `cells` cells -> their means; a non-finite cell in any channel makes all of them NaN
// (fg_planebudgets.hip keeps these lines in its kernel: through this function its 15 / 18 means were allocated to other registers)
template <int K>
__device__ __forceinline__ void finish_means(double (&mu)[K], double cells) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        mu[k] = mu[k] / cells;
        bad = bad || !(fabs(mu[k]) <= DBL_MAX);
    }
    if (bad) {
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] = (double)NAN;
    }
}

// order-2 merge of one central sum: A, B the sums of d_i d_j of the record and of the sample, w2 = nA nB / n
__device__ __forceinline__ double merge2(double A, double B, double dl_i, double dl_j, double w2) { return A + B + dl_i * dl_j * w2; }

// every row of env b has read n[b] before it takes its ticket (a 64-bit integer atomic, acquire / release at device scope); the row
// that draws the last ticket of this call's ny rows stores the new n.  a: the kernel's arguments with tickets, n and ny.  A macro for
// the reason given at FG_ROWSTAT_OWN_ROW: as a function, by value or by reference, it changed the code of one kernel file or the other.
#define FG_ROWSTAT_ADVANCE_N(a, b, n_new)                                                                                              \
    do {                                                                                                                               \
        const unsigned long long ticket = __hip_atomic_fetch_add(&(a).tickets[b], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);   \
        if ((ticket + 1ull) % (unsigned long long)(a).ny == 0ull) (a).n[b] = (n_new);                                                  \
    } while (0)

// the channels of a launch, by value in the kernel arguments: no pointer table in device memory, no copy per call
template <int MAXK>
struct ChannelTable {
    const fg_real* ch[MAXK];
    long long bstride[MAXK];
};

// t from the caller's tables with their checks; vec: 16-byte loads are allowed.  `entry` names the extern "C" function and `what`
// its pointers ("channel", "field") in the messages.
template <int MAXK>
int fill(ChannelTable<MAXK>& t, bool& vec, const char* entry, const char* what, const fg_real* const* ptrs, const int64_t* batch_stride,
         int K, int nz, int ny, int nx) {
    const std::string e(entry);
    const long long field = (long long)nz * ny * nx;
    vec = nx % VEC == 0;
    for (int k = 0; k < MAXK; ++k) {
        t.ch[k] = nullptr; t.bstride[k] = 0;
        if (k >= K) continue;
        FG_REQUIRE(ptrs[k], FG_ERR_INVALID_ARG, e + ": null " + what + " pointer");
        FG_REQUIRE(batch_stride[k] >= field, FG_ERR_INVALID_ARG, e + ": batch stride smaller than nz * ny * nx");
        t.ch[k] = ptrs[k]; t.bstride[k] = (long long)batch_stride[k];
        vec = vec && ((uintptr_t)ptrs[k] % 16 == 0) && (batch_stride[k] % VEC == 0);
    }
    return FG_OK;
}

// fill for a recorder that owns rows: the extents one launch takes first
template <int MAXK>
int fill_rows(ChannelTable<MAXK>& t, bool& vec, const char* entry, const char* what, const fg_real* const* ptrs,
              const int64_t* batch_stride, int K, int batch, int nz, int ny, int nx) {
    const std::string e(entry);
    FG_REQUIRE((long long)nz * nx <= (1LL << 30), FG_ERR_INVALID_ARG, e + ": a plane of more than 2^30 cells");
    FG_REQUIRE((long long)batch * ny <= 0x7fffffffLL, FG_ERR_INVALID_ARG, e + ": batch * ny too large for one launch");
    return fill(t, vec, entry, what, ptrs, batch_stride, K, nz, ny, nx);
}

// f(grid, V, WAVE) with the load width and the ownership form of a launch as std::integral_constant
template <typename F>
void launch(long long rows, bool vec, bool wave, F&& f) {
    const dim3 grid((unsigned)(wave ? (rows + 3) / 4 : rows));
    using one = std::integral_constant<int, 1>;
    using wide = std::integral_constant<int, VEC>;
    if (vec) {
        if (wave) f(grid, wide{}, std::true_type{});
        else f(grid, wide{}, std::false_type{});
    } else {
        if (wave) f(grid, one{}, std::true_type{});
        else f(grid, one{}, std::false_type{});
    }
}

}  // namespace fg_rowstat
