// Online temporal two-point correlations of wall-parallel planes (PlaneTimeCorrelation, simulation/plane_timecorr.py): per
// wall-normal row (env, y) and channel the correlation of the plane's fluctuation with the fluctuation the same plane had a number
// of samples ago, for a ring of stored base fluctuations.
//
// The reference keeps this with TemporalTwoPointCorrelation_Online_torch (pict/data/online_statistics.py:1271-1343; fed by
// TCF_tools.VelocityStats.record_vel_stats :1508-1511): one cloned base field of one realisation, per sample a torch.mean, a
// full-field difference, three more means and a division.  Here one sample of a batch of B envs is ONE launch, whatever the number
// of live bases:
//   pass 1   the plane sum of a channel of a row, fp64                                          -> the sample's mean
//   pass 2   the same cells again (they sit in L2 / MALL from pass 1), c' = value - mean in fp64, the sums of c'^2 and of b' c' for
//            the stored base b' of every live slot; a slot at lag 0 gets c' rounded to fg_real stored as its base and takes its
//            sum of b'^2 and its cross term from the rounded values, so that lag 0 and the later lags see the same base
//   add      coefficient, cross / cells, base variance, current variance into acc [row][k][lag][4]; when one of the three sums is not
//            finite (a non-finite cell in the sample or in the stored base) all four become NaN: an entry is whole or lost
//
// Registers: the channels of a row are taken one after the other (a run-time loop around both passes), the live slots inside the
// cell loop (a template parameter).  A thread then carries 2 + L fp64 partial sums and (1 + L) loads in flight, not K (2 + L): with
// K = 5 and L = 8 that is 10 sums instead of 50 (100 VGPRs), and the kernel is instantiated 8 times per load width and ownership
// form instead of 40 times.  A channel's plane is re-read while it is the only thing the workgroup touches.
//
// Ownership, order and the loads are those of fg_rowstat.h; every accumulator element and every base cell is written by exactly
// one thread.
#include <float.h>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int PT_MAX_K = 5;
constexpr int PT_MAX_SLOTS = 8;

struct PtArgs {
    rs::ChannelTable<PT_MAX_K> t;
    long long zstride, rows, field;      // ny * nx; batch * ny; nz * ny * nx
    int nz, ny, nx, K, batch, lags;
    int slot[PT_MAX_SLOTS], lag[PT_MAX_SLOTS];   // the live slots of this sample; with `store`, entry 0 is the slot at lag 0
    int store;
    fg_real* base;
    double* base_ss;
    double* acc;
};

// v rounded to fg_real, stored at p and handed back as what a later load will see
template <int VEC>
__device__ __forceinline__ void pt_store(fg_real* p, double (&v)[VEC]) {
    fg_real r[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { r[j] = (fg_real)v[j]; v[j] = (double)r[j]; }
    if constexpr (VEC == 1) {
        p[0] = r[0];
    } else {
#if FG_F64
        *reinterpret_cast<double2*>(p) = make_double2(r[0], r[1]);
#else
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
#endif
    }
}

template <int L, int VEC, bool WAVE>
__global__ __launch_bounds__(256) void k_plane_timecorr(PtArgs a) {
    constexpr int M = L + 2;                                 // sum c'^2, sum b'^2 of the slot being stored, L cross terms
    __shared__ double s_red[4][M];
    const int tid = threadIdx.x;
    FG_ROWSTAT_OWN_ROW(a, VEC, WAVE, tid);
    const double cells = (double)a.nz * (double)a.nx;
    const bool store = a.store != 0;

    for (int k = 0; k < a.K; ++k) {
        const fg_real* src = a.t.ch[k] + (long long)b * a.t.bstride[k] + (long long)y * a.nx;
        fg_real* bp[L];
#pragma unroll
        for (int j = 0; j < L; ++j) bp[j] = a.base + (((long long)a.slot[j] * a.batch + b) * a.K + k) * a.field + (long long)y * a.nx;

        double mu[1] = {0.0};
        for (int i = t0; i < items; i += step) {
            const int z = i / nxv, xv = i - z * nxv;
            double v[VEC];
            rs::load<VEC>(src + (long long)z * a.zstride + (long long)xv * VEC, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) mu[0] += v[j];
        }
        rs::reduce<1, M, WAVE>(mu, s_red, tid);
        const double mean = mu[0] / cells;

        double s[M];
#pragma unroll
        for (int q = 0; q < M; ++q) s[q] = 0.0;
        for (int i = t0; i < items; i += step) {
            const long long off = rs::item_offset<VEC>(i, nxv, a.zstride);
            double c[VEC], bv[L][VEC];
            rs::load<VEC>(src + off, c);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                if (j > 0 || !store) rs::load<VEC>(bp[j] + off, bv[j]);
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) c[j] -= mean;
            if (store) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) bv[0][j] = c[j];
                pt_store<VEC>(bp[0] + off, bv[0]);
#pragma unroll
                for (int j = 0; j < VEC; ++j) s[1] += bv[0][j] * bv[0][j];
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                s[0] += c[j] * c[j];
#pragma unroll
                for (int q = 0; q < L; ++q) s[2 + q] += bv[q][j] * c[j];
            }
        }
        rs::reduce<M, M, WAVE>(s, s_red, tid);

        if (t0 == 0) {
            double* ga = a.acc + (row * a.K + k) * (long long)a.lags * 4;
#pragma unroll
            for (int j = 0; j < L; ++j) {
                double* ss = a.base_ss + (((long long)a.slot[j] * a.batch + b) * a.ny + y) * a.K + k;
                double bb;
                if (j == 0 && store) { bb = s[1]; *ss = bb; }
                else bb = *ss;
                double* g = ga + (long long)a.lag[j] * 4;
                double add[4] = {s[2 + j] / sqrt(bb * s[0]), s[2 + j] / cells, bb / cells, s[0] / cells};
                // a non-finite cell in the sample or in the base: the pair is lost, all four entries of its lag say so
                if (!(fabs(s[2 + j]) <= DBL_MAX && fabs(bb) <= DBL_MAX && fabs(s[0]) <= DBL_MAX)) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) add[q] = (double)NAN;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) g[q] += add[q];
            }
        }
    }
}

template <int L>
void pt_launch(const PtArgs& a, bool vec, bool wave, hipStream_t st) {
    rs::launch(a.rows, vec, wave, [&](dim3 grid, auto v, auto w) {
        hipLaunchKernelGGL((k_plane_timecorr<L, decltype(v)::value, decltype(w)::value>), grid, dim3(256), 0, st, a);
    });
}

}  // namespace

extern "C" int fg_plane_timecorr(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz,
                                 int32_t ny, int32_t nx, int32_t lags, int32_t n_slots, const int32_t* slot_lag, fg_real* base,
                                 double* base_ss, double* acc, void* stream) {
    FG_REQUIRE(channels && batch_stride && slot_lag, FG_ERR_INVALID_ARG, "fg_plane_timecorr: null channel, stride or slot table");
    FG_REQUIRE(base && base_ss && acc, FG_ERR_INVALID_ARG, "fg_plane_timecorr: null base, base_ss or acc");
    FG_REQUIRE(K >= 1 && K <= PT_MAX_K, FG_ERR_INVALID_ARG, "fg_plane_timecorr: K must be 1..5");
    FG_REQUIRE(lags >= 1, FG_ERR_INVALID_ARG, "fg_plane_timecorr: lags must be positive");
    FG_REQUIRE(n_slots >= 1 && n_slots <= PT_MAX_SLOTS, FG_ERR_INVALID_ARG, "fg_plane_timecorr: n_slots must be 1..8");
    FG_REQUIRE(batch > 0 && nz > 0 && ny > 0 && nx > 0, FG_ERR_INVALID_ARG, "fg_plane_timecorr: batch, nz, ny, nx must be positive");
    const long long field = (long long)nz * ny * nx;
    PtArgs a;
    bool vec;
    const int rc = rs::fill_rows(a.t, vec, "fg_plane_timecorr", "channel", channels, batch_stride, K, batch, nz, ny, nx);
    if (rc != FG_OK) return rc;
    vec = vec && (uintptr_t)base % 16 == 0;
    // the live slots, the one at lag 0 first
    int live = 0;
    a.store = 0;
    for (int j = 0; j < PT_MAX_SLOTS; ++j) { a.slot[j] = 0; a.lag[j] = 0; }
    for (int pass = 0; pass < 2; ++pass) {
        for (int j = 0; j < n_slots; ++j) {
            const int l = slot_lag[j];
            if (pass == 0) {
                FG_REQUIRE(l >= -1 && l < lags, FG_ERR_INVALID_ARG, "fg_plane_timecorr: a slot_lag entry outside [-1, lags)");
                for (int i = 0; i < j; ++i)
                    FG_REQUIRE(l < 0 || slot_lag[i] != l, FG_ERR_INVALID_ARG, "fg_plane_timecorr: two slots with the same lag");
            }
            if (l < 0 || (l == 0) != (pass == 0)) continue;
            a.slot[live] = j; a.lag[live] = l; ++live;
            if (l == 0) a.store = 1;
        }
    }
    if (live == 0) return FG_OK;                             // every slot idle: nothing to record
    a.zstride = (long long)ny * nx; a.rows = (long long)batch * ny; a.field = field;
    a.nz = nz; a.ny = ny; a.nx = nx; a.K = K; a.batch = batch; a.lags = lags;
    a.base = base; a.base_ss = base_ss; a.acc = acc;
    const bool wave = (long long)nz * nx <= rs::WAVE_CELLS;
    hipStream_t st = (hipStream_t)stream;
    switch (live) {
        case 1: pt_launch<1>(a, vec, wave, st); break;
        case 2: pt_launch<2>(a, vec, wave, st); break;
        case 3: pt_launch<3>(a, vec, wave, st); break;
        case 4: pt_launch<4>(a, vec, wave, st); break;
        case 5: pt_launch<5>(a, vec, wave, st); break;
        case 6: pt_launch<6>(a, vec, wave, st); break;
        case 7: pt_launch<7>(a, vec, wave, st); break;
        default: pt_launch<8>(a, vec, wave, st); break;
    }
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
