// Online plane-averaged flow statistics (PlaneMoments, simulation/plane_stats.py): per wall-normal row (env, y) the mean of K
// channels over the homogeneous directions (z, x) and the sums of products of deviations up to order 4, merged over the samples
// of a run on the device.
//
// The reference keeps these with WelfordOnlineParallel_Torch / CovarianceOnlineParallel_Torch / MultivariateMomentsOnlineParallel_Torch
// (pict/data/online_statistics.py:31-266, 419-787; fed by TCF_tools.VelocityStats.record_vel_stats :1480-1507): per statistic a
// torch.mean over the field, a full-field difference and a torch.sum.  Here one sample of a batch of B envs is ONE launch:
//   pass 1   the plane sums of the K channels of a row, fp64                                   -> the sample's mean
//   pass 2   the same cells again (they sit in L2 / MALL from pass 1: a plane is at most a few hundred KB), the sums of
//            d_i d_j (i <= j), d_i^3, d_i^4 of the deviations d = value - mean, fp64            -> the sample's central sums
//   merge    with the running accumulators by the pairwise update of Pebay et al. 2016 (delta = mean_sample - mean_running; at
//            order 2 the parallel Welford / Schubert-Gertz rule); a first sample (n = 0) is stored
//
// Ownership and order: one workgroup of 256 threads owns a row whose plane has more than PM_WAVE_CELLS cells (the TCF shape
// 8 x 128 x 64 x 64: 512 rows of 128 x 64 cells), one wave of a four-wave workgroup a smaller one (2-D fields: a plane is one x row,
// so a workgroup takes four y rows).  Every lane adds its cells in ascending order, the lanes combine by the xor butterfly of the
// wave, the waves in ascending order through LDS: a fixed tree, no floating-point atomic anywhere, so a row's result depends on
// nothing but the row's cells and the extents.
//
// n[env] is read by every row of the env and advanced once per call: the rows take a ticket (a 64-bit integer atomic, acquire /
// release at device scope) after they have read n, and the row that draws the last ticket of the call stores the new n.
#include <float.h>

#include "fg_internal.h"

namespace {

constexpr int PM_MAX_K = 5;
constexpr int PM_WAVE_CELLS = 1024;      // planes up to this many cells are reduced by one wave
constexpr int PM_VEC = FG_F64 ? 2 : 4;   // reals per 16-byte load

struct PmArgs {
    const fg_real* ch[PM_MAX_K];         // by value: no pointer table in device memory, no copy per call
    long long bstride[PM_MAX_K];
    long long zstride, rows;             // ny * nx; batch * ny
    int nz, ny, nx;
    double* n;
    double* mean;
    double* central;
    unsigned long long* tickets;
};

template <int VEC>
__device__ __forceinline__ void pm_load(const fg_real* p, double (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = (double)p[0];
    } else {
#if FG_F64
        const double2 q = *reinterpret_cast<const double2*>(p);
        v[0] = q.x; v[1] = q.y;
#else
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
#endif
    }
}

// the sum of v[q] over the lanes of the wave (WAVE) or of the workgroup, left in every lane: xor butterfly, then the four waves in
// ascending order
template <int N, int S, bool WAVE>
__device__ __forceinline__ void pm_reduce(double (&v)[N], double (&s_red)[4][S], int tid) {
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

template <int K, int ORDER, int VEC, bool WAVE>
__global__ __launch_bounds__(256) void k_plane_moments(PmArgs a) {
    constexpr int P = K * (K + 1) / 2;
    constexpr int M = P + (ORDER >= 3 ? K : 0) + (ORDER >= 4 ? K : 0);
    __shared__ double s_red[4][M];
    const int tid = threadIdx.x;
    const long long row = WAVE ? (long long)blockIdx.x * 4 + (tid >> 6) : (long long)blockIdx.x;
    if (WAVE && row >= a.rows) return;                       // a whole wave; this form has no barrier
    const int b = (int)(row / a.ny), y = (int)(row - (long long)b * a.ny);
    const int nxv = a.nx / VEC, items = a.nz * nxv;
    const int t0 = WAVE ? (tid & 63) : tid, step = WAVE ? 64 : 256;
    const fg_real* base[K];
#pragma unroll
    for (int k = 0; k < K; ++k) base[k] = a.ch[k] + (long long)b * a.bstride[k] + (long long)y * a.nx;

    double mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.0;
    for (int i = t0; i < items; i += step) {
        const int z = i / nxv, xv = i - z * nxv;
        const long long off = (long long)z * a.zstride + (long long)xv * VEC;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v[VEC];
            pm_load<VEC>(base[k] + off, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) mu[k] += v[j];
        }
    }
    pm_reduce<K, M, WAVE>(mu, s_red, tid);
    const double cells = (double)a.nz * (double)a.nx;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        mu[k] = mu[k] / cells;
        bad = bad || !(fabs(mu[k]) <= DBL_MAX);
    }
    if (bad) {                                               // a non-finite cell in any channel: the whole sample of this row is NaN
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] = (double)NAN;
    }

    double c[M];
#pragma unroll
    for (int q = 0; q < M; ++q) c[q] = 0.0;
    for (int i = t0; i < items; i += step) {
        const int z = i / nxv, xv = i - z * nxv;
        const long long off = (long long)z * a.zstride + (long long)xv * VEC;
        double d[K][VEC];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            pm_load<VEC>(base[k] + off, d[k]);
#pragma unroll
            for (int j = 0; j < VEC; ++j) d[k][j] -= mu[k];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            int q = 0;
#pragma unroll
            for (int i1 = 0; i1 < K; ++i1) {
#pragma unroll
                for (int i2 = i1; i2 < K; ++i2) c[q++] += d[i1][j] * d[i2][j];
            }
            if constexpr (ORDER >= 3) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double d2 = d[k][j] * d[k][j];
                    c[P + k] += d2 * d[k][j];
                    if constexpr (ORDER >= 4) c[P + K + k] += d2 * d2;
                }
            }
        }
    }
    pm_reduce<M, M, WAVE>(c, s_red, tid);
    if (t0 != 0) return;

    // ---- merge: A = the running record, B = this sample, delta = mean_B - mean_A (Pebay et al. 2016, eq. 3.1 without weights)
    const double nA = a.n[b], nB = cells, n = nA + nB;
    double* gm = a.mean + row * K;
    double* gc = a.central + row * M;
    if (nA == 0.0) {
#pragma unroll
        for (int k = 0; k < K; ++k) gm[k] = mu[k];
#pragma unroll
        for (int q = 0; q < M; ++q) gc[q] = c[q];
    } else {
        double dl[K], a2[K], b2[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double mA = gm[k];
            dl[k] = mu[k] - mA;
            gm[k] = (nA * mA + nB * mu[k]) / n;
        }
        const double w2 = nA * nB / n;
        int q = 0;
#pragma unroll
        for (int i1 = 0; i1 < K; ++i1) {
#pragma unroll
            for (int i2 = i1; i2 < K; ++i2) {
                const double A = gc[q];
                if (i1 == i2) { a2[i1] = A; b2[i1] = c[q]; }
                gc[q] = A + c[q] + dl[i1] * dl[i2] * w2;
                ++q;
            }
        }
        if constexpr (ORDER >= 3) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double A3 = gc[P + k], B3 = c[P + k], dk = dl[k], dk2 = dk * dk;
                gc[P + k] = A3 + B3 + dk2 * dk * (nA * nB * (nA - nB) / (n * n)) + 3.0 * dk * ((nA * b2[k] - nB * a2[k]) / n);
                if constexpr (ORDER >= 4) {
                    const double A4 = gc[P + K + k], B4 = c[P + K + k];
                    gc[P + K + k] = A4 + B4 + dk2 * dk2 * (nA * nB * (nA * nA - nA * nB + nB * nB) / (n * n * n))
                                    + 6.0 * dk2 * ((nA * nA * b2[k] + nB * nB * a2[k]) / (n * n)) + 4.0 * dk * ((nA * B3 - nB * A3) / n);
                }
            }
        }
    }
    // every row of env b has read n[b] before it takes its ticket; the last one of this call's ny rows advances n[b]
    const unsigned long long ticket = __hip_atomic_fetch_add(&a.tickets[b], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if ((ticket + 1ull) % (unsigned long long)a.ny == 0ull) a.n[b] = n;
}

template <int K, int ORDER>
void pm_launch(const PmArgs& a, bool vec, bool wave, hipStream_t st) {
    const dim3 grid((unsigned)(wave ? (a.rows + 3) / 4 : a.rows));
    if (vec) {
        if (wave) hipLaunchKernelGGL((k_plane_moments<K, ORDER, PM_VEC, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_plane_moments<K, ORDER, PM_VEC, false>), grid, dim3(256), 0, st, a);
    } else {
        if (wave) hipLaunchKernelGGL((k_plane_moments<K, ORDER, 1, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_plane_moments<K, ORDER, 1, false>), grid, dim3(256), 0, st, a);
    }
}

template <int K>
void pm_launch_order(const PmArgs& a, int order, bool vec, bool wave, hipStream_t st) {
    if (order == 2) pm_launch<K, 2>(a, vec, wave, st);
    else if (order == 3) pm_launch<K, 3>(a, vec, wave, st);
    else pm_launch<K, 4>(a, vec, wave, st);
}

}  // namespace

extern "C" int fg_plane_moments(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz,
                                int32_t ny, int32_t nx, int32_t order, double* n, double* mean, double* central, uint64_t* tickets,
                                void* stream) {
    FG_REQUIRE(channels && batch_stride, FG_ERR_INVALID_ARG, "fg_plane_moments: null channel table or stride table");
    FG_REQUIRE(n && mean && central && tickets, FG_ERR_INVALID_ARG, "fg_plane_moments: null accumulator (n, mean, central, tickets)");
    FG_REQUIRE(K >= 3 && K <= PM_MAX_K, FG_ERR_INVALID_ARG, "fg_plane_moments: K must be 3..5");
    FG_REQUIRE(order >= 2 && order <= 4, FG_ERR_INVALID_ARG, "fg_plane_moments: order must be 2..4");
    FG_REQUIRE(batch > 0 && nz > 0 && ny > 0 && nx > 0, FG_ERR_INVALID_ARG, "fg_plane_moments: batch, nz, ny, nx must be positive");
    FG_REQUIRE((long long)nz * nx <= (1LL << 30), FG_ERR_INVALID_ARG, "fg_plane_moments: a plane of more than 2^30 cells");
    FG_REQUIRE((long long)batch * ny <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_plane_moments: batch * ny too large for one launch");
    const long long field = (long long)nz * ny * nx;
    PmArgs a;
    bool vec = nx % PM_VEC == 0;
    for (int k = 0; k < PM_MAX_K; ++k) {
        a.ch[k] = nullptr; a.bstride[k] = 0;
        if (k >= K) continue;
        FG_REQUIRE(channels[k], FG_ERR_INVALID_ARG, "fg_plane_moments: null channel pointer");
        FG_REQUIRE(batch_stride[k] >= field, FG_ERR_INVALID_ARG, "fg_plane_moments: batch stride smaller than nz * ny * nx");
        a.ch[k] = channels[k]; a.bstride[k] = (long long)batch_stride[k];
        vec = vec && ((uintptr_t)channels[k] % 16 == 0) && (batch_stride[k] % PM_VEC == 0);
    }
    a.zstride = (long long)ny * nx; a.rows = (long long)batch * ny;
    a.nz = nz; a.ny = ny; a.nx = nx;
    a.n = n; a.mean = mean; a.central = central; a.tickets = (unsigned long long*)tickets;
    const bool wave = (long long)nz * nx <= PM_WAVE_CELLS;
    hipStream_t st = (hipStream_t)stream;
    if (K == 3) pm_launch_order<3>(a, order, vec, wave, st);
    else if (K == 4) pm_launch_order<4>(a, order, vec, wave, st);
    else pm_launch_order<5>(a, order, vec, wave, st);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
