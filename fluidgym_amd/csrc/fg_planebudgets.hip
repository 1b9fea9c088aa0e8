// Online Reynolds-stress budgets of channel flows (PlaneBudgets, simulation/plane_budgets.py): per wall-normal row (env, y) the means
// over the homogeneous directions (z, x) of K = 15 channels -- u, v, w, the pressure gradient, the nine velocity gradients; 18 with
// the forcing s -- and the M = 43 (52) sums of products of their deviations that the terms of the Reynolds-stress transport equation
// are made of, merged over the samples of a run on the device.
//
// The reference keeps these with TurbulentEnergyBudgetsOnlineParallel_Torch (pict/data/online_statistics.py:790-1268): twelve
// full-field padded differences and about fifty torch.mean / torch.sum passes per sample.  Here one sample of a batch of B envs is ONE
// launch, the gradients never leave the registers:
//   gradient the reference's _data_grad(borders="ZERO"): (f[i+1] - f[i-1]) / |pos[i+1] - pos[i-1]| with the ghost position mirrored
//            (2 pos[0] - pos[1]) and the ghost value 0, on every axis; on x and z a `wrap` flag takes the ghost VALUE from the other end
//            of the axis instead (the ghost distance stays the mirrored one).  Row y reads rows y - 1 and y + 1 of its env from L2.
//   pass 1   the plane sums of the K channels of a row, fp64                                   -> the sample's means
//   pass 2   the same cells again, the M sums of products of deviations, fp64                   -> the sample's central sums
//   merge    with the running accumulators by the pairwise update of Pebay et al. 2016 (delta = mean_sample - mean_running), mixed
//            third-order sums included; a first sample (n = 0) is stored
//
// Channels: 0..2 u, v, w; 3..5 dp/dx, dp/dy, dp/dz; 6 + 3 k + i = d u_i / d x_k; with forcing 15..17 s_x, s_y, s_z.
// Central sums (budget_keys of plane_budgets.py): the 6 second-order sums of (u, v, w) (i <= j), the 10 third-order ones
// (i <= j <= k), the 9 u_i dp/dx_j (i, then j), with forcing the 9 u_i s_j, then per direction k the 6 second-order sums of
// (d_k u, d_k v, d_k w).
//
// Ownership, order, the loads and the ticket for n[env] are those of fg_rowstat.h; a row's result depends on nothing but the row's
// cells, its two neighbour rows, the coordinates and the extents.  A non-finite value in any channel of a row -- a non-finite cell of
// the row itself or, through d/dy, of a neighbour row -- makes the sample of that row NaN.
#include <float.h>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int PB_MAX_FIELDS = 7;         // u, v, w, p, s_x, s_y, s_z

struct PbArgs {
    rs::ChannelTable<PB_MAX_FIELDS> t;
    long long zstride, rows;             // ny * nx; batch * ny
    int nz, ny, nx;
    int wrap_x, wrap_z;
    const double* x;
    const double* y;
    const double* z;
    double* n;
    double* mean;
    double* central;
    unsigned long long* tickets;
};

// 1 / |pos[i + 1] - pos[i - 1]| with mirrored ghost positions at both ends (n >= 2)
__device__ __forceinline__ double pb_rdist(const double* pos, int i, int n) {
    const double lo = i > 0 ? pos[i - 1] : 2.0 * pos[0] - pos[1];
    const double hi = i < n - 1 ? pos[i + 1] : 2.0 * pos[n - 1] - pos[n - 2];
    return 1.0 / fabs(hi - lo);
}

// what one work item (VEC consecutive cells in x of the row) reads: the cells themselves, their neighbours in y and z as vectors, the
// two neighbours in x beyond the ends of the vector as scalars.  A ghost is 0.
template <int NF, int VEC>
struct PbItem {
    fg_real c[NF][VEC];
    fg_real ym[4][VEC], yp[4][VEC], zm[4][VEC], zp[4][VEC];
    fg_real xm[4], xp[4];
    double rx[VEC], rz;
};

template <int NF, int VEC>
__device__ __forceinline__ void pb_read(const PbArgs& a, const fg_real* const (&base)[NF], int y, int z, int x0, PbItem<NF, VEC>& it) {
    const long long off = (long long)z * a.zstride + x0;
#pragma unroll
    for (int f = 0; f < NF; ++f) rs::load<VEC>(base[f] + off, it.c[f]);
    // z - 1, z + 1, x0 - 1, x0 + VEC: an offset, or no read at all
    const bool has_zm = z > 0 || a.wrap_z, has_zp = z < a.nz - 1 || a.wrap_z;
    const long long ozm = z > 0 ? off - a.zstride : off + (long long)(a.nz - 1) * a.zstride;
    const long long ozp = z < a.nz - 1 ? off + a.zstride : off - (long long)(a.nz - 1) * a.zstride;
    const bool has_xm = x0 > 0 || a.wrap_x, has_xp = x0 + VEC < a.nx || a.wrap_x;
    const long long oxm = x0 > 0 ? off - 1 : off + (a.nx - 1);
    const long long oxp = x0 + VEC < a.nx ? off + VEC : off + VEC - a.nx;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) it.ym[f][j] = it.yp[f][j] = it.zm[f][j] = it.zp[f][j] = (fg_real)0;
        if (y > 0) rs::load<VEC>(base[f] + off - a.nx, it.ym[f]);
        if (y < a.ny - 1) rs::load<VEC>(base[f] + off + a.nx, it.yp[f]);
        if (has_zm) rs::load<VEC>(base[f] + ozm, it.zm[f]);
        if (has_zp) rs::load<VEC>(base[f] + ozp, it.zp[f]);
        it.xm[f] = has_xm ? base[f][oxm] : (fg_real)0;
        it.xp[f] = has_xp ? base[f][oxp] : (fg_real)0;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) it.rx[j] = pb_rdist(a.x, x0 + j, a.nx);
    it.rz = pb_rdist(a.z, z, a.nz);
}

// the K channels of cell j of an item, fp64; differences of the values as they were cast
template <int NF, int VEC, int K>
__device__ __forceinline__ void pb_channels(const PbItem<NF, VEC>& it, int j, double ry, double (&ch)[K]) {
    double gx[4], gy[4], gz[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const double lo = (double)(j > 0 ? it.c[f][j > 0 ? j - 1 : 0] : it.xm[f]);
        const double hi = (double)(j < VEC - 1 ? it.c[f][j < VEC - 1 ? j + 1 : 0] : it.xp[f]);
        gx[f] = (hi - lo) * it.rx[j];
        gy[f] = ((double)it.yp[f][j] - (double)it.ym[f][j]) * ry;
        gz[f] = ((double)it.zp[f][j] - (double)it.zm[f][j]) * it.rz;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ch[i] = (double)it.c[i][j];
        ch[6 + i] = gx[i];
        ch[9 + i] = gy[i];
        ch[12 + i] = gz[i];
        if constexpr (NF == 7) ch[15 + i] = (double)it.c[4 + i][j];
    }
    ch[3] = gx[3]; ch[4] = gy[3]; ch[5] = gz[3];
}

__device__ __forceinline__ constexpr int pb_pair(int i, int j) {      // index of the second-order sum (i <= j) of (u, v, w)
    return i == 0 ? j : (i == 1 ? 2 + j : 5);
}

template <int NF, int VEC, bool WAVE>
__global__ __launch_bounds__(256) void k_plane_budgets(PbArgs a) {
    constexpr bool F = NF == 7;
    constexpr int K = F ? 18 : 15;
    constexpr int Q3 = 6, QP = 16, QS = 25, QG = F ? 34 : 25, M = QG + 18;
    __shared__ double s_red[4][M];
    const int tid = threadIdx.x;
    FG_ROWSTAT_OWN_ROW(a, VEC, WAVE, tid);
    const fg_real* base[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) base[f] = a.t.ch[f] + (long long)b * a.t.bstride[f] + (long long)y * a.nx;
    const double ry = pb_rdist(a.y, y, a.ny);

    double mu[K];
#pragma unroll
    for (int k = 0; k < K; ++k) mu[k] = 0.0;
    for (int i = t0; i < items; i += step) {
        const int z = i / nxv, xv = i - z * nxv;
        PbItem<NF, VEC> it;
        pb_read<NF, VEC>(a, base, y, z, xv * VEC, it);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double ch[K];
            pb_channels<NF, VEC, K>(it, j, ry, ch);
#pragma unroll
            for (int k = 0; k < K; ++k) mu[k] += ch[k];
        }
    }
    rs::reduce<K, M, WAVE>(mu, s_red, tid);
    const double cells = (double)a.nz * (double)a.nx;
    bool bad = false;                                        // (not rs::finish_means: with it the register allocation of this kernel changes)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        mu[k] = mu[k] / cells;
        bad = bad || !(fabs(mu[k]) <= DBL_MAX);
    }
    if (bad) {                                               // a non-finite value in any channel: the whole sample of this row is NaN
#pragma unroll
        for (int k = 0; k < K; ++k) mu[k] = (double)NAN;
    }

    double c[M];
#pragma unroll
    for (int q = 0; q < M; ++q) c[q] = 0.0;
    for (int i = t0; i < items; i += step) {
        const int z = i / nxv, xv = i - z * nxv;
        PbItem<NF, VEC> it;
        pb_read<NF, VEC>(a, base, y, z, xv * VEC, it);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double d[K];
            pb_channels<NF, VEC, K>(it, j, ry, d);
#pragma unroll
            for (int k = 0; k < K; ++k) d[k] -= mu[k];
            int q2 = 0, q3 = Q3;
#pragma unroll
            for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
                for (int i2 = i1; i2 < 3; ++i2) {
                    const double p2 = d[i1] * d[i2];
                    c[q2++] += p2;
#pragma unroll
                    for (int i3 = i2; i3 < 3; ++i3) c[q3++] += p2 * d[i3];
                }
            }
#pragma unroll
            for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
                for (int i2 = 0; i2 < 3; ++i2) {
                    c[QP + 3 * i1 + i2] += d[i1] * d[3 + i2];
                    if constexpr (F) c[QS + 3 * i1 + i2] += d[i1] * d[15 + i2];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                int q = QG + 6 * k;
#pragma unroll
                for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
                    for (int i2 = i1; i2 < 3; ++i2) c[q++] += d[6 + 3 * k + i1] * d[6 + 3 * k + i2];
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
        double dl[K], a2[6];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double mA = gm[k];
            dl[k] = mu[k] - mA;
            gm[k] = (nA * mA + nB * mu[k]) / n;
        }
        const double w2 = nA * nB / n, w3 = nA * nB * (nA - nB) / (n * n);
        int q2 = 0, q3 = Q3;
#pragma unroll
        for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
            for (int i2 = i1; i2 < 3; ++i2) {
                a2[q2] = gc[q2];
                gc[q2] = rs::merge2(a2[q2], c[q2], dl[i1], dl[i2], w2);
                ++q2;
            }
        }
#pragma unroll
        for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
            for (int i2 = i1; i2 < 3; ++i2) {
#pragma unroll
                for (int i3 = i2; i3 < 3; ++i3) {
                    const int p23 = pb_pair(i2, i3), p13 = pb_pair(i1, i3), p12 = pb_pair(i1, i2);
                    gc[q3] = gc[q3] + c[q3] + dl[i1] * dl[i2] * dl[i3] * w3
                             + (dl[i1] * (nA * c[p23] - nB * a2[p23]) + dl[i2] * (nA * c[p13] - nB * a2[p13])
                                + dl[i3] * (nA * c[p12] - nB * a2[p12])) / n;
                    ++q3;
                }
            }
        }
#pragma unroll
        for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
            for (int i2 = 0; i2 < 3; ++i2) {
                const int qp = QP + 3 * i1 + i2;
                gc[qp] = rs::merge2(gc[qp], c[qp], dl[i1], dl[3 + i2], w2);
                if constexpr (F) {
                    const int qs = QS + 3 * i1 + i2;
                    gc[qs] = rs::merge2(gc[qs], c[qs], dl[i1], dl[15 + i2], w2);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int q = QG + 6 * k;
#pragma unroll
            for (int i1 = 0; i1 < 3; ++i1) {
#pragma unroll
                for (int i2 = i1; i2 < 3; ++i2) {
                    gc[q] = rs::merge2(gc[q], c[q], dl[6 + 3 * k + i1], dl[6 + 3 * k + i2], w2);
                    ++q;
                }
            }
        }
    }
    FG_ROWSTAT_ADVANCE_N(a, b, n);
}

template <int NF>
void pb_launch(const PbArgs& a, bool vec, bool wave, hipStream_t st) {
    rs::launch(a.rows, vec, wave, [&](dim3 grid, auto v, auto w) {
        hipLaunchKernelGGL((k_plane_budgets<NF, decltype(v)::value, decltype(w)::value>), grid, dim3(256), 0, st, a);
    });
}

}  // namespace

extern "C" int fg_plane_budgets(const fg_real* const* fields, const int64_t* batch_stride, int32_t n_fields, int32_t batch, int32_t nz,
                                int32_t ny, int32_t nx, const double* x, const double* y, const double* z, int32_t wrap_x,
                                int32_t wrap_z, double* n, double* mean, double* central, uint64_t* tickets, void* stream) {
    FG_REQUIRE(fields && batch_stride, FG_ERR_INVALID_ARG, "fg_plane_budgets: null field table or stride table");
    FG_REQUIRE(x && y && z, FG_ERR_INVALID_ARG, "fg_plane_budgets: null coordinate array (x, y, z)");
    FG_REQUIRE(n && mean && central && tickets, FG_ERR_INVALID_ARG, "fg_plane_budgets: null accumulator (n, mean, central, tickets)");
    FG_REQUIRE(n_fields == 4 || n_fields == PB_MAX_FIELDS, FG_ERR_INVALID_ARG,
               "fg_plane_budgets: n_fields must be 4 (u, v, w, p) or 7 (with the forcing s_x, s_y, s_z)");
    FG_REQUIRE(batch > 0, FG_ERR_INVALID_ARG, "fg_plane_budgets: batch must be positive");
    FG_REQUIRE(nz >= 2 && ny >= 2 && nx >= 2, FG_ERR_INVALID_ARG, "fg_plane_budgets: nz, ny, nx must be at least 2 (a central difference)");
    PbArgs a;
    bool vec;
    const int rc = rs::fill_rows(a.t, vec, "fg_plane_budgets", "field", fields, batch_stride, n_fields, batch, nz, ny, nx);
    if (rc != FG_OK) return rc;
    a.zstride = (long long)ny * nx; a.rows = (long long)batch * ny;
    a.nz = nz; a.ny = ny; a.nx = nx;
    a.wrap_x = wrap_x != 0; a.wrap_z = wrap_z != 0;
    a.x = x; a.y = y; a.z = z;
    a.n = n; a.mean = mean; a.central = central; a.tickets = (unsigned long long*)tickets;
    const bool wave = (long long)nz * nx <= rs::WAVE_CELLS;
    hipStream_t st = (hipStream_t)stream;
    if (n_fields == 4) pb_launch<4>(a, vec, wave, st);
    else pb_launch<7>(a, vec, wave, st);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
