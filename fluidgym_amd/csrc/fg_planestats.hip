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
// Ownership and order (one workgroup or one wave per row, a fixed reduction tree), the loads and the ticket that advances n[env]
// once per call are those of fg_rowstat.h.
#include <float.h>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int PM_MAX_K = 5;

struct PmArgs {
    rs::ChannelTable<PM_MAX_K> t;
    long long zstride, rows;             // ny * nx; batch * ny
    int nz, ny, nx;
    double* n;
    double* mean;
    double* central;
    unsigned long long* tickets;
};

template <int K, int ORDER, int VEC, bool WAVE>
__global__ __launch_bounds__(256) void k_plane_moments(PmArgs a) {
    constexpr int P = K * (K + 1) / 2;
    constexpr int M = P + (ORDER >= 3 ? K : 0) + (ORDER >= 4 ? K : 0);
    __shared__ double s_red[4][M];
    const int tid = threadIdx.x;
    FG_ROWSTAT_OWN_ROW(a, VEC, WAVE, tid);
    const fg_real* base[K];
#pragma unroll
    for (int k = 0; k < K; ++k) base[k] = a.t.ch[k] + (long long)b * a.t.bstride[k] + (long long)y * a.nx;

    double mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.0;
    for (int i = t0; i < items; i += step) {
        const long long off = rs::item_offset<VEC>(i, nxv, a.zstride);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v[VEC];
            rs::load<VEC>(base[k] + off, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) mu[k] += v[j];
        }
    }
    rs::reduce<K, M, WAVE>(mu, s_red, tid);
    const double cells = (double)a.nz * (double)a.nx;
    rs::finish_means<K>(mu, cells);                          // a non-finite cell in any channel: the whole sample of this row is NaN

    double c[M];
#pragma unroll
    for (int q = 0; q < M; ++q) c[q] = 0.0;
    for (int i = t0; i < items; i += step) {
        const long long off = rs::item_offset<VEC>(i, nxv, a.zstride);
        double d[K][VEC];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rs::load<VEC>(base[k] + off, d[k]);
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
    rs::reduce<M, M, WAVE>(c, s_red, tid);
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
                gc[q] = rs::merge2(A, c[q], dl[i1], dl[i2], w2);
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
    FG_ROWSTAT_ADVANCE_N(a, b, n);
}

template <int K, int ORDER>
void pm_launch(const PmArgs& a, bool vec, bool wave, hipStream_t st) {
    rs::launch(a.rows, vec, wave, [&](dim3 grid, auto v, auto w) {
        hipLaunchKernelGGL((k_plane_moments<K, ORDER, decltype(v)::value, decltype(w)::value>), grid, dim3(256), 0, st, a);
    });
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
    PmArgs a;
    bool vec;
    const int rc = rs::fill_rows(a.t, vec, "fg_plane_moments", "channel", channels, batch_stride, K, batch, nz, ny, nx);
    if (rc != FG_OK) return rc;
    a.zstride = (long long)ny * nx; a.rows = (long long)batch * ny;
    a.nz = nz; a.ny = ny; a.nx = nx;
    a.n = n; a.mean = mean; a.central = central; a.tickets = (unsigned long long*)tickets;
    const bool wave = (long long)nz * nx <= rs::WAVE_CELLS;
    hipStream_t st = (hipStream_t)stream;
    if (K == 3) pm_launch_order<3>(a, order, vec, wave, st);
    else if (K == 4) pm_launch_order<4>(a, order, vec, wave, st);
    else pm_launch_order<5>(a, order, vec, wave, st);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
