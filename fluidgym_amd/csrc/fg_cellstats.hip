// Online per-cell flow statistics of the multi-block domains (CellMoments, simulation/cell_moments.py): per column -- a cell of a
// 2-D mesh, the nz cells (block, :, y, x) along the periodic span of a 3-D one -- the mean of the K = d + 1 channels u, v(, w), p and
// the K (K + 1) / 2 sums of products of deviations from it, merged over the samples of a run on the device.
//
// The reference keeps these with WelfordOnlineParallel_Torch / CovarianceOnlineParallel_Torch (pict/data/online_statistics.py:31-266)
// per block, dims = [0] in 2-D and [0, 2] in 3-D: per statistic and block a torch.mean, a full-field difference and a torch.sum.
// Here one sample of a batch of B envs is ONE launch over the flat fields velocity [B, d, N], pressure [B, N] as MultiBlockDomain
// holds them (blocks contiguous in N, x fastest, z slowest):
//   pass 1   the sums of the K channels over the column's nz cells, ascending z, fp64          -> the sample's mean
//   pass 2   the same cells again (just read: L1 / L2), the sums of d_i d_j (i <= j), fp64     -> the sample's central sums
//   merge    with the running accumulators mean [B][K][NC], central [B][K (K + 1) / 2][NC] by the order-2 rule of fg_rowstat.h
//            (parallel Welford / Schubert-Gertz, delta = mean_sample - mean_running), n_A = samples * nz, n_B = nz; the first
//            sample (samples = 0) is stored.  `samples` is a kernel argument: the host counts, the device keeps no counter.
//
// Ownership and order: a thread owns a column -- in a block whose offsets allow 16-byte loads CM_VEC neighbouring columns, each in
// registers of its own -- and neighbouring lanes own neighbouring x, so the loads of the fields and the 8-byte accesses of every
// accumulator plane coalesce.  No floating-point atomic, no cross-lane operation: a column's result depends on its own cells and
// `samples` only.  The arithmetic of a column is written once (cm_column) and this file is compiled with -ffp-contract=off (its own
// rule in the Makefile; the build's -ffp-contract=fast would fuse products into the sums and ignores a pragma): every product and
// sum is rounded on its own, so both load forms, any batch and any launch give the same bits, and they are the bits of the NumPy
// twin.  The block table travels by value in the kernel arguments.
#include <float.h>
#include <limits.h>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int CM_MAX_BLOCKS = 8;
constexpr int CM_VEC = rs::VEC;

struct CmBlock {
    long long cell_offset, column_offset, item_offset;   // item: what one thread owns, `width` neighbouring columns
    int layer_cells, nz, width;
};

struct CmArgs {
    const fg_real* velocity;             // [B][d][N]
    const fg_real* pressure;             // [B][N]
    long long N, NC, items, samples;
    double* mean;
    double* central;
    CmBlock blk[CM_MAX_BLOCKS];          // by value: no table in device memory, no copy per call
};

// W neighbouring accumulators of one plane: 8-byte accesses for one column, 16-byte ones for an aligned group
template <int W>
__device__ __forceinline__ void cm_acc_load(const double* p, double (&v)[W]) {
    if constexpr (W == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int j = 0; j < W; j += 2) {
            const double2 q = *reinterpret_cast<const double2*>(p + j);
            v[j] = q.x; v[j + 1] = q.y;
        }
    }
}

template <int W>
__device__ __forceinline__ void cm_acc_store(double* p, const double (&v)[W]) {
    if constexpr (W == 1) {
        p[0] = v[0];
    } else {
#pragma unroll
        for (int j = 0; j < W; j += 2) *reinterpret_cast<double2*>(p + j) = make_double2(v[j], v[j + 1]);
    }
}

// the columns col .. col + W - 1 of one block of env b
template <int K, int W>
__device__ __forceinline__ void cm_column(const CmArgs& a, int b, long long cell_offset, long long column_offset, int layer_cells, int nz,
                                          long long col) {
    constexpr int P = K * (K + 1) / 2;
    const fg_real* base[K];
#pragma unroll
    for (int k = 0; k < K - 1; ++k) base[k] = a.velocity + ((long long)b * (K - 1) + k) * a.N + cell_offset + col;
    base[K - 1] = a.pressure + (long long)b * a.N + cell_offset + col;

    double mu[K][W];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < W; ++j) mu[k][j] = 0.0;
    }
    for (int z = 0; z < nz; ++z) {
        const long long off = (long long)z * layer_cells;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v[W];
            rs::load<W>(base[k] + off, v);
#pragma unroll
            for (int j = 0; j < W; ++j) mu[k][j] += v[j];
        }
    }
    const double nB = (double)nz;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        bool bad = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            mu[k][j] = mu[k][j] / nB;
            bad = bad || !(fabs(mu[k][j]) <= DBL_MAX);
        }
        if (bad) {                                           // a non-finite cell in any channel: the whole sample of this column is NaN
#pragma unroll
            for (int k = 0; k < K; ++k) mu[k][j] = (double)NAN;
        }
    }

    double c[P][W];
#pragma unroll
    for (int q = 0; q < P; ++q) {
#pragma unroll
        for (int j = 0; j < W; ++j) c[q][j] = 0.0;
    }
    for (int z = 0; z < nz; ++z) {
        const long long off = (long long)z * layer_cells;
        double d[K][W];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            rs::load<W>(base[k] + off, d[k]);
#pragma unroll
            for (int j = 0; j < W; ++j) d[k][j] -= mu[k][j];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            int q = 0;
#pragma unroll
            for (int i1 = 0; i1 < K; ++i1) {
#pragma unroll
                for (int i2 = i1; i2 < K; ++i2) {
                    c[q][j] += d[i1][j] * d[i2][j];
                    ++q;
                }
            }
        }
    }

    // ---- merge: A = the running record, B = this sample, delta = mean_B - mean_A
    double* gm = a.mean + (long long)b * K * a.NC + column_offset + col;
    double* gc = a.central + (long long)b * P * a.NC + column_offset + col;
    if (a.samples == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) cm_acc_store<W>(gm + (long long)k * a.NC, mu[k]);
#pragma unroll
        for (int q = 0; q < P; ++q) cm_acc_store<W>(gc + (long long)q * a.NC, c[q]);
        return;
    }
    const double nA = (double)a.samples * nB, n = nA + nB, w2 = nA * nB / n;
    double dl[K][W];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double mA[W];
        cm_acc_load<W>(gm + (long long)k * a.NC, mA);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            dl[k][j] = mu[k][j] - mA[j];
            mA[j] = (nA * mA[j] + nB * mu[k][j]) / n;
        }
        cm_acc_store<W>(gm + (long long)k * a.NC, mA);
    }
    int q = 0;
#pragma unroll
    for (int i1 = 0; i1 < K; ++i1) {
#pragma unroll
        for (int i2 = i1; i2 < K; ++i2) {
            double A[W];
            cm_acc_load<W>(gc + (long long)q * a.NC, A);
#pragma unroll
            for (int j = 0; j < W; ++j) A[j] = rs::merge2(A[j], c[q][j], dl[i1][j], dl[i2][j], w2);
            cm_acc_store<W>(gc + (long long)q * a.NC, A);
            ++q;
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_mb_cell_moments(CmArgs a) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= a.items) return;
    // the block of this item: the table is indexed by constants only (selects, no copy of it to scratch); unused entries start at
    // LLONG_MAX
    long long cell_offset = a.blk[0].cell_offset, column_offset = a.blk[0].column_offset, item_offset = a.blk[0].item_offset;
    int layer_cells = a.blk[0].layer_cells, nz = a.blk[0].nz, width = a.blk[0].width;
#pragma unroll
    for (int i = 1; i < CM_MAX_BLOCKS; ++i) {
        if (item >= a.blk[i].item_offset) {
            cell_offset = a.blk[i].cell_offset; column_offset = a.blk[i].column_offset; item_offset = a.blk[i].item_offset;
            layer_cells = a.blk[i].layer_cells; nz = a.blk[i].nz; width = a.blk[i].width;
        }
    }
    const long long col = (item - item_offset) * width;
    if (width == 1) cm_column<K, 1>(a, (int)blockIdx.y, cell_offset, column_offset, layer_cells, nz, col);
    else cm_column<K, CM_VEC>(a, (int)blockIdx.y, cell_offset, column_offset, layer_cells, nz, col);
}

// the block table of the launch from the host table: checks, the columns, and per block what a thread owns.  16-byte accesses need
// the field pointers and the planes of both accumulators 16-byte aligned for every env and channel, and per block the first cell,
// the layer and the first column
int cm_plan(CmArgs& a, const int64_t* block_table, int n_blocks) {
    const long long n_cells = a.N;
    long long columns = 0;
    for (int i = 0; i < n_blocks; ++i) {                     // rows of (cell_offset, layer_cells, nz, column_offset)
        const int64_t* r = block_table + 4 * i;
        FG_REQUIRE(r[1] > 0 && r[2] > 0, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: layer_cells and nz of a block must be positive");
        FG_REQUIRE(r[1] <= n_cells && r[2] <= n_cells && r[1] * r[2] <= n_cells && r[0] >= 0 && r[0] <= n_cells - r[1] * r[2],
                   FG_ERR_INVALID_ARG, "fg_mb_cell_moments: the cells of a block lie outside the field");
        FG_REQUIRE(r[3] == columns, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: column_offset must be the columns of the blocks before");
        columns += r[1];
    }
    a.NC = columns;
    const bool vec_all = (uintptr_t)a.velocity % 16 == 0 && (uintptr_t)a.pressure % 16 == 0 && n_cells % CM_VEC == 0 &&
                         (uintptr_t)a.mean % 16 == 0 && (uintptr_t)a.central % 16 == 0 && columns % CM_VEC == 0;
    long long items = 0;
    for (int i = 0; i < CM_MAX_BLOCKS; ++i) {
        CmBlock& k = a.blk[i];
        if (i >= n_blocks) {
            k.cell_offset = k.column_offset = 0; k.item_offset = LLONG_MAX; k.layer_cells = k.nz = k.width = 1;
            continue;
        }
        const int64_t* r = block_table + 4 * i;
        const bool vec = vec_all && r[0] % CM_VEC == 0 && r[1] % CM_VEC == 0 && r[3] % CM_VEC == 0;
        k.cell_offset = r[0]; k.layer_cells = (int)r[1]; k.nz = (int)r[2]; k.column_offset = r[3];
        k.width = vec ? CM_VEC : 1;
        k.item_offset = items;
        items += r[1] / k.width;
    }
    a.items = items;
    return FG_OK;
}

}  // namespace

#define CM_CHECK_ARGS                                                                                                                     \
    FG_REQUIRE(velocity && pressure && block_table, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: null velocity, pressure or block table");   \
    FG_REQUIRE(mean && central, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: null accumulator (mean, central)");                              \
    FG_REQUIRE(n_cells > 0 && n_cells <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: n_cells must be 1..2^31 - 1");            \
    FG_REQUIRE(n_blocks >= 1 && n_blocks <= CM_MAX_BLOCKS, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: n_blocks must be 1..8")

extern "C" int fg_mb_cell_moments_widths(const fg_real* velocity, const fg_real* pressure, int64_t n_cells, const int64_t* block_table,
                                         int32_t n_blocks, const double* mean, const double* central, int32_t* widths) {
    CM_CHECK_ARGS;
    FG_REQUIRE(widths, FG_ERR_INVALID_ARG, "fg_mb_cell_moments_widths: null widths");
    CmArgs a;
    a.velocity = velocity; a.pressure = pressure; a.N = n_cells; a.samples = 0; a.mean = (double*)mean; a.central = (double*)central;
    const int rc = cm_plan(a, block_table, n_blocks);
    if (rc != FG_OK) return rc;
    for (int i = 0; i < n_blocks; ++i) widths[i] = a.blk[i].width;
    return FG_OK;
}

extern "C" int fg_mb_cell_moments(const fg_real* velocity, const fg_real* pressure, int32_t dims, int32_t batch, int64_t n_cells,
                                  const int64_t* block_table, int32_t n_blocks, int64_t samples, double* mean, double* central,
                                  void* stream) {
    CM_CHECK_ARGS;
    FG_REQUIRE(dims == 2 || dims == 3, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: dims must be 2 or 3");
    FG_REQUIRE(batch > 0 && batch <= 65535, FG_ERR_INVALID_ARG, "fg_mb_cell_moments: batch must be 1..65535");
    FG_REQUIRE(samples >= 0 && samples < (1LL << 40), FG_ERR_INVALID_ARG, "fg_mb_cell_moments: samples must be 0..2^40 - 1");
    CmArgs a;
    a.velocity = velocity; a.pressure = pressure; a.N = n_cells; a.samples = samples; a.mean = mean; a.central = central;
    const int rc = cm_plan(a, block_table, n_blocks);
    if (rc != FG_OK) return rc;
    const dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (dims == 2) hipLaunchKernelGGL((k_mb_cell_moments<3>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_mb_cell_moments<4>), grid, dim3(256), 0, st, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
