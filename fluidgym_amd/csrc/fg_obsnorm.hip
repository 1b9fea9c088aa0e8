// Running normalisation of the observations and rewards of a batch (include/fluidgym_hip.h): the record (n, mean, M2)
// of every statistic slot is advanced by the selected rows of this call and every row is normalised with the record after the update.
// n is a host integer and comes by value; mean and M2 are fp64 on the device.  All arithmetic below is fp64, every product, sum and
// division rounded on its own (the file is compiled with -ffp-contract=off); the result is rounded once to the tensor's dtype.
//
//     mean_b = sum_{r in R} x[r] / m;   M2_b = sum_{r in R} (x[r] - mean_b)^2          two passes over the selected rows R, m = |R|
//     delta  = mean_b - mean_a;  n = n_a + m;  mean = mean_a + delta * (m / n);  M2 = M2_a + M2_b + (delta * delta) * (n_a * m / n)
//     (an empty record, n_a = 0, is read as mean_a = M2_a = 0 whatever the memory holds: the merge then returns the batch exactly)
//     rstd   = 1 / sqrt(M2 / n + epsilon);   y = (x - mean) * rstd,  clipped to [-clip, clip] where clip > 0
//
// THE ORDER OF EVERY SUM is a function of (m, n = elements per row, pooled) alone -- not of the load form, the addresses, the number of
// rows that are only normalised, or the timing.  There is no floating-point atomic.
//
//   Element slots (one per element of a row).  L = min(1024, max(4, the power of two >= m)) row lanes, CQ = max(1, 256 / L) quad
//   columns (a quad is four consecutive elements) and T = L * CQ threads per workgroup (256, 512 or 1024).  The workgroup owns the CQ
//   quads from blockIdx.x * CQ; thread t is quad column t % CQ and row lane l = t / CQ.  For each of its four elements on its own:
//     1. lane l starts at 0.0 and adds the selected rows k = l, l + L, l + 2 L, ... < m in ascending order (k counts the selected rows;
//        row_list[k] is the row);
//     2. the 64 / CQ row lanes of a wave combine by the xor butterfly over the lane distances 32, 16, ..., CQ (none where CQ = 64);
//     3. the T / 64 waves are added in ascending order, ((w0 + w1) + w2) + ..., through LDS.
//   The same tree sums x and then (x - mean_b)^2.  Statistics, merge and normalisation of a column happen in the one workgroup that
//   owns it, so the whole dict is ONE launch and no workgroup waits for another.  Few rows of many elements (64 x 2 048) give L = 64,
//   CQ = 4: 128 workgroups, one row per lane; many rows of few elements (16 384 x 30) give L = 1024, CQ = 1: one workgroup of 1024
//   lanes per quad, 16 rows per lane.
//
//   A pooled slot (one per key, over the rows and the elements: m n values).  One workgroup of 1024 threads owns the key.  With
//   Q = ceil(n / 4) quads per row, thread t takes the items i = t, t + 1024, ... < m Q in ascending order, item i being quad i % Q of
//   selected row i / Q, and adds the elements of an item in ascending order, starting at 0.0; then the xor butterfly over the lane
//   distances 32 ... 1 and the 16 waves in ascending order.  That is a launch of its own (reduce and merge); the normalisation
//   follows in the launch of the element slots, which reads the merged record: two launches, never more.
//
//   The return record of the rewards (fg_obs_return_normalize): one workgroup of 1024 threads; thread t takes the rows t, t + 1024,
//   ... in ascending order; butterfly 32 ... 1; 16 waves ascending.  G[r] = gamma * G[r] + reward[r] first, then the two passes over
//   G, the merge into stats = {mean, M2}, and after the barrier out[r] = reward[r] * rstd (no mean subtraction), clipped.
//
// Loads and stores: a quad by 16-byte words where both bases, both row pitches and the position in the row allow it, element by
// element otherwise (and for the tail quad of a row); the values and the arithmetic are the same.  dst == src is allowed: a workgroup
// has read every selected row of its columns (the barrier of the reduction) before it stores to them.  Nothing returns to the host,
// nothing is allocated.
#include "fg_internal.h"

namespace {

constexpr int NORM_MAX_SEG = 8;
constexpr int NORM_MAX_N = 1 << 26;
constexpr int NORM_MAX_THREADS = 1024;
constexpr int NORM_MAX_WAVES = NORM_MAX_THREADS / 64;

struct NormSeg {
    const void* src;
    void* dst;
    long long src_stride, dst_stride;     // elements between rows
    double* mean;                         // [n], or [1] pooled
    double* m2;
    int n;                                // elements per row
    int vec;                              // both bases and both row pitches are multiples of 16 bytes
    int pooled;
    int stats;                            // this launch advances the record of the segment (element slots, updating)
};

struct NormArgs {
    NormSeg seg[NORM_MAX_SEG];
    const int32_t* row_list;              // [m] ascending rows, or null: row k is k
    int rows, m;                          // rows normalised, rows merged
    int cq;                               // quad columns per workgroup (a power of two <= 64)
    double n_a, n_total;                  // rows in the record before / after this call
    double epsilon, clip;
};

// the quad at p as doubles: `left` (1..4) elements of it exist
template <typename T>
__device__ __forceinline__ void load_quad(const T* p, bool wide, int left, double (&v)[4]) {
    if (wide) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(p);
            v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
        } else {
            const double2 lo = reinterpret_cast<const double2*>(p)[0], hi = reinterpret_cast<const double2*>(p)[1];
            v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < left ? (double)p[j] : 0.0;
    }
}

template <typename T>
__device__ __forceinline__ void store_quad(T* p, bool wide, int left, const double (&v)[4]) {
    if (wide) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        } else {
            reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]);
            reinterpret_cast<double2*>(p)[1] = make_double2(v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) p[j] = (T)v[j];
    }
}

// the sums of v[0..K) over the threads of the workgroup that share tid % cq, left in each of them: butterfly over the lane distances
// 32 ... cq, then the waves in ascending order.  Two barriers: every load before the call is done before any store after it.
template <int K>
__device__ __forceinline__ void reduce_columns(double (&v)[K], double (*s_red)[K][64], int tid, int cq, int waves) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        for (int off = 32; off >= cq; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
    }
    const int lane = tid & 63, col = lane & (cq - 1);
    if (lane < cq) {
#pragma unroll
        for (int q = 0; q < K; ++q) s_red[tid >> 6][q][lane] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        double s = s_red[0][q][col];
        for (int w = 1; w < waves; ++w) s = s + s_red[w][q][col];
        v[q] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void merge_record(double mean_a, double m2_a, double mean_b, double m2_b, double n_a, double m, double& mean,
                                             double& m2) {
    const double n = n_a + m;
    const double delta = mean_b - mean_a;
    mean = mean_a + delta * (m / n);
    m2 = m2_a + m2_b + (delta * delta) * (n_a * m / n);
}

__device__ __forceinline__ double normalized(double x, double mean, double rstd, double clip) {
    double y = (x - mean) * rstd;
    if (clip > 0.0) y = fmin(fmax(y, -clip), clip);
    return y;
}

// element slots: statistics, merge and normalisation of the columns a workgroup owns; pooled or frozen segments are only normalised
template <typename T>
__global__ __launch_bounds__(NORM_MAX_THREADS) void k_obs_normalize(const NormArgs a) {
    __shared__ double s_red[NORM_MAX_WAVES][4][64];
    const NormSeg& sg = a.seg[blockIdx.y];                       // wave-uniform
    const int cq = a.cq;
    if (4LL * blockIdx.x * cq >= sg.n) return;                   // the whole workgroup: a shorter segment of the dict
    const int tid = threadIdx.x, T_ = blockDim.x;
    const int L = T_ / cq, l = tid / cq;
    const long long i0 = 4LL * ((long long)blockIdx.x * cq + (tid & (cq - 1)));
    const int left = (int)(sg.n - i0 < 4 ? (sg.n - i0 < 0 ? 0 : sg.n - i0) : 4);   // 0: a column past the end of the row
    const bool wide = sg.vec && left == 4;
    const T* src = static_cast<const T*>(sg.src) + i0;
    T* dst = static_cast<T*>(sg.dst) + i0;

    double mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};
    const bool have = sg.stats ? a.n_a > 0.0 : true;             // an empty record is not read
    if (have) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < left) {
                const long long slot = sg.pooled ? 0 : i0 + j;
                mean[j] = sg.mean[slot];
                m2[j] = sg.m2[slot];
            }
        }
    }
    if (sg.stats) {
        const double m = (double)a.m;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (left > 0) {
            for (int k = l; k < a.m; k += L) {
                const long long r = a.row_list ? a.row_list[k] : k;
                double v[4];
                load_quad(src + r * sg.src_stride, wide, left, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = s[j] + v[j];
            }
        }
        reduce_columns<4>(s, s_red, tid, cq, T_ >> 6);
        double mean_b[4], d2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) mean_b[j] = s[j] / m;
        if (left > 0) {
            for (int k = l; k < a.m; k += L) {
                const long long r = a.row_list ? a.row_list[k] : k;
                double v[4];
                load_quad(src + r * sg.src_stride, wide, left, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = v[j] - mean_b[j];
                    d2[j] = d2[j] + d * d;
                }
            }
        }
        reduce_columns<4>(d2, s_red, tid, cq, T_ >> 6);
#pragma unroll
        for (int j = 0; j < 4; ++j) merge_record(mean[j], m2[j], mean_b[j], d2[j], a.n_a, m, mean[j], m2[j]);
        if (l == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < left) {
                    sg.mean[i0 + j] = mean[j];
                    sg.m2[i0 + j] = m2[j];
                }
            }
        }
    }
    if (left <= 0) return;
    const double count = sg.pooled ? a.n_total * (double)sg.n : a.n_total;
    double rstd[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rstd[j] = 1.0 / sqrt(m2[j] / count + a.epsilon);
    for (int r = l; r < a.rows; r += L) {
        double v[4];
        load_quad(src + (long long)r * sg.src_stride, wide, left, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = normalized(v[j], mean[j], rstd[j], a.clip);
        store_quad(dst + (long long)r * sg.dst_stride, wide, left, v);
    }
}

// pooled slots: one workgroup per key reduces the selected rows and merges the scalar record
template <typename T>
__global__ __launch_bounds__(NORM_MAX_THREADS) void k_obs_pool_stats(const NormArgs a) {
    __shared__ double s_red[NORM_MAX_WAVES][1][64];
    const NormSeg& sg = a.seg[blockIdx.x];
    if (!sg.pooled) return;
    const int tid = threadIdx.x;
    const unsigned Q = (unsigned)((sg.n + 3) / 4), items = (unsigned)a.m * Q;      // the entry keeps m * Q below 2^31
    const T* src = static_cast<const T*>(sg.src);
    const double mean_a = a.n_a > 0.0 ? sg.mean[0] : 0.0, m2_a = a.n_a > 0.0 ? sg.m2[0] : 0.0;
    const double count = (double)a.m * (double)sg.n;
    double mean_b = 0.0;
    double acc[1];
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        acc[0] = 0.0;
        for (unsigned i = (unsigned)tid; i < items; i += NORM_MAX_THREADS) {
            const unsigned k = i / Q, q = i - k * Q;
            const long long r = a.row_list ? a.row_list[k] : (long long)k;
            const int left = (int)(sg.n - 4 * (int)q < 4 ? sg.n - 4 * (int)q : 4);
            double v[4];
            load_quad(src + r * sg.src_stride + 4LL * q, sg.vec && left == 4, left, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < left) {
                    if (pass == 0) {
                        acc[0] = acc[0] + v[j];
                    } else {
                        const double d = v[j] - mean_b;
                        acc[0] = acc[0] + d * d;
                    }
                }
            }
        }
        reduce_columns<1>(acc, s_red, tid, 1, NORM_MAX_WAVES);
        if (pass == 0) mean_b = acc[0] / count;
    }
    if (tid == 0) {
        double mean, m2;
        merge_record(mean_a, m2_a, mean_b, acc[0], a.n_a * (double)sg.n, count, mean, m2);
        sg.mean[0] = mean;
        sg.m2[0] = m2;
    }
}

struct ReturnArgs {
    const void* reward;
    void* out;
    double* G;
    double* stats;                        // {mean, M2}
    int rows, update;
    double gamma, n_a, epsilon, clip;
};

template <typename T>
__global__ __launch_bounds__(NORM_MAX_THREADS) void k_obs_return_normalize(const ReturnArgs a) {
    __shared__ double s_red[NORM_MAX_WAVES][1][64];
    const int tid = threadIdx.x;
    const T* reward = static_cast<const T*>(a.reward);
    T* out = static_cast<T*>(a.out);
    double mean = 0.0, m2 = 0.0;
    if (a.n_a > 0.0) { mean = a.stats[0]; m2 = a.stats[1]; }
    double acc[1] = {0.0};
    for (int r = tid; r < a.rows; r += NORM_MAX_THREADS) {
        const double g = a.gamma * a.G[r] + (double)reward[r];
        a.G[r] = g;
        acc[0] = acc[0] + g;
    }
    double count = a.n_a;
    if (a.update) {                                              // uniform
        const double m = (double)a.rows;
        reduce_columns<1>(acc, s_red, tid, 1, NORM_MAX_WAVES);
        const double mean_b = acc[0] / m;
        acc[0] = 0.0;
        for (int r = tid; r < a.rows; r += NORM_MAX_THREADS) {   // the G this thread stored
            const double d = a.G[r] - mean_b;
            acc[0] = acc[0] + d * d;
        }
        reduce_columns<1>(acc, s_red, tid, 1, NORM_MAX_WAVES);
        merge_record(mean, m2, mean_b, acc[0], a.n_a, m, mean, m2);
        count = a.n_a + m;
        if (tid == 0) { a.stats[0] = mean; a.stats[1] = m2; }
    }
    const double rstd = 1.0 / sqrt(m2 / count + a.epsilon);
    for (int r = tid; r < a.rows; r += NORM_MAX_THREADS) {
        double y = (double)reward[r] * rstd;
        if (a.clip > 0.0) y = fmin(fmax(y, -a.clip), a.clip);
        out[r] = (T)y;
    }
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

extern "C" int fg_obs_normalize(const fg_norm_segment* seg, int32_t n_seg, int32_t rows, int32_t dtype, int64_t n_before, int64_t n_add,
                                const int32_t* row_list, int32_t n_rows_sel, int32_t update, double epsilon, double clip, void* stream) {
    const std::string e = "fg_obs_normalize: ";
    FG_REQUIRE(seg, FG_ERR_INVALID_ARG, e + "null argument (seg is required)");
    FG_REQUIRE(n_seg >= 1 && n_seg <= NORM_MAX_SEG, FG_ERR_INVALID_ARG,
               e + "n_seg = " + std::to_string(n_seg) + " is outside [1, " + std::to_string(NORM_MAX_SEG) + "]");
    FG_REQUIRE(rows >= 1 && rows <= 65535, FG_ERR_INVALID_ARG, e + "rows = " + std::to_string(rows) + " is outside [1, 65535]");
    FG_REQUIRE(dtype == 0 || dtype == 1, FG_ERR_INVALID_ARG, e + "dtype must be 0 (float) or 1 (double)");
    FG_REQUIRE(n_before >= 0 && n_before <= (1LL << 52), FG_ERR_INVALID_ARG,
               e + "n_before = " + std::to_string(n_before) + " is outside [0, 2^52]");
    FG_REQUIRE(epsilon > 0.0, FG_ERR_INVALID_ARG, e + "epsilon must be positive");
    if (row_list)
        FG_REQUIRE(n_rows_sel >= 1 && n_rows_sel <= rows, FG_ERR_INVALID_ARG,
                   e + "n_rows_sel = " + std::to_string(n_rows_sel) + " is outside [1, rows = " + std::to_string(rows) + "]");
    const int m = row_list ? n_rows_sel : rows;
    if (update) {
        FG_REQUIRE(n_add == m, FG_ERR_INVALID_ARG,
                   e + "n_add = " + std::to_string(n_add) + " where the call merges " + std::to_string(m) + " rows");
    } else {
        FG_REQUIRE(n_add == 0, FG_ERR_INVALID_ARG, e + "n_add = " + std::to_string(n_add) + " where a frozen call (update = 0) merges nothing");
        FG_REQUIRE(n_before > 0, FG_ERR_INVALID_ARG, e + "update = 0 with n_before = 0: an empty record cannot normalise");
    }
    const size_t elem = dtype == 0 ? 4 : 8;
    NormArgs a{};
    int max_n = 0;
    bool any_pooled = false;
    for (int32_t s = 0; s < n_seg; ++s) {
        const fg_norm_segment& g = seg[s];
        const std::string who = e + "segment " + std::to_string(s);
        FG_REQUIRE(g.src && g.dst && g.mean && g.m2, FG_ERR_INVALID_ARG, who + ": null src, dst, mean or m2");
        FG_REQUIRE(g.n >= 1 && g.n <= NORM_MAX_N, FG_ERR_INVALID_ARG, who + ": n = " + std::to_string(g.n) + " is outside [1, 2^26]");
        FG_REQUIRE(g.src_stride >= g.n && g.dst_stride >= g.n, FG_ERR_INVALID_ARG,
                   who + ": a stride (" + std::to_string(g.src_stride) + ", " + std::to_string(g.dst_stride) + ") is smaller than n = " +
                       std::to_string(g.n));
        FG_REQUIRE(g.pooled == 0 || g.pooled == 1, FG_ERR_INVALID_ARG, who + ": pooled must be 0 or 1");
        if (g.pooled && update)
            FG_REQUIRE((long long)m * ((g.n + 3) / 4) < (1LL << 31), FG_ERR_INVALID_ARG,
                       who + ": a pooled update of " + std::to_string(m) + " rows x n = " + std::to_string(g.n) + " exceeds 2^31 quads");
        NormSeg& k = a.seg[s];
        k.src = g.src; k.dst = g.dst; k.src_stride = g.src_stride; k.dst_stride = g.dst_stride;
        k.mean = g.mean; k.m2 = g.m2; k.n = g.n; k.pooled = g.pooled;
        k.stats = (update && !g.pooled) ? 1 : 0;
        k.vec = (reinterpret_cast<uintptr_t>(g.src) % 16 == 0 && reinterpret_cast<uintptr_t>(g.dst) % 16 == 0 &&
                 ((size_t)g.src_stride * elem) % 16 == 0 && ((size_t)g.dst_stride * elem) % 16 == 0) ? 1 : 0;
        max_n = g.n > max_n ? g.n : max_n;
        any_pooled = any_pooled || g.pooled;
    }
    a.row_list = row_list; a.rows = rows; a.m = m;
    a.n_a = (double)n_before; a.n_total = (double)(n_before + n_add);
    a.epsilon = epsilon; a.clip = clip;
    // the shape of a launch: a function of m alone (the order rule at the top of the file)
    const int L = std::min(NORM_MAX_THREADS, std::max(4, pow2_at_least(m)));
    a.cq = std::max(1, 256 / L);
    const unsigned threads = (unsigned)(L * a.cq);
    if (update && any_pooled) {
        if (dtype == 0) hipLaunchKernelGGL(k_obs_pool_stats<float>, dim3((unsigned)n_seg), dim3(NORM_MAX_THREADS), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(k_obs_pool_stats<double>, dim3((unsigned)n_seg), dim3(NORM_MAX_THREADS), 0, (hipStream_t)stream, a);
        FG_HIP_CHECK(hipGetLastError());
    }
    const unsigned quads = (unsigned)((max_n + 3) / 4);
    const dim3 grid((quads + a.cq - 1) / a.cq, (unsigned)n_seg);
    if (dtype == 0) hipLaunchKernelGGL(k_obs_normalize<float>, grid, dim3(threads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_obs_normalize<double>, grid, dim3(threads), 0, (hipStream_t)stream, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_obs_return_normalize(const void* reward, void* out, double* G, double* stats, int32_t rows, int32_t dtype, double gamma,
                                       int64_t n_before, double epsilon, double clip, int32_t update, void* stream) {
    const std::string e = "fg_obs_return_normalize: ";
    FG_REQUIRE(reward && out && G && stats, FG_ERR_INVALID_ARG, e + "null argument (reward, out, G and stats are required)");
    FG_REQUIRE(rows >= 1 && rows <= 65535, FG_ERR_INVALID_ARG, e + "rows = " + std::to_string(rows) + " is outside [1, 65535]");
    FG_REQUIRE(dtype == 0 || dtype == 1, FG_ERR_INVALID_ARG, e + "dtype must be 0 (float) or 1 (double)");
    FG_REQUIRE(gamma >= 0.0 && gamma <= 1.0, FG_ERR_INVALID_ARG, e + "gamma = " + std::to_string(gamma) + " is outside [0, 1]");
    FG_REQUIRE(n_before >= 0 && n_before <= (1LL << 52), FG_ERR_INVALID_ARG,
               e + "n_before = " + std::to_string(n_before) + " is outside [0, 2^52]");
    FG_REQUIRE(epsilon > 0.0, FG_ERR_INVALID_ARG, e + "epsilon must be positive");
    FG_REQUIRE(update || n_before > 0, FG_ERR_INVALID_ARG, e + "update = 0 with n_before = 0: an empty record cannot normalise");
    ReturnArgs a{};
    a.reward = reward; a.out = out; a.G = G; a.stats = stats; a.rows = rows; a.update = update ? 1 : 0;
    a.gamma = gamma; a.n_a = (double)n_before; a.epsilon = epsilon; a.clip = clip;
    if (dtype == 0) hipLaunchKernelGGL(k_obs_return_normalize<float>, dim3(1), dim3(NORM_MAX_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_obs_return_normalize<double>, dim3(1), dim3(NORM_MAX_THREADS), 0, (hipStream_t)stream, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
