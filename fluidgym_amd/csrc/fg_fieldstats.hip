// Field summaries for the domain statistics (FluidEnv.compute_domain_statistics): per-env moments and a per-env histogram of one
// component, or of the Euclidean magnitude, of a contiguous device field [batch, channels, n].
//
// The reference keeps, per env type, a Stats record (mean, min, max, five percentiles) of velocity magnitude and pressure over an
// uncontrolled rollout (fluid_env.py:33-47, 1192-1221); the generator of those records is not part of its package.  Here one
// sample of a batch of B envs is one launch pair:
//   moments    min / max / count over the finite cells, their sum, the count of non-finite cells -- per env
//   histogram  uniform bins over [lo, lo + nbins * width), 64-bit counts, ADDED to the caller's array -- per env
// Everything that crosses a workgroup is an integer: min / max travel as order-preserving 64-bit keys through atomicMin /
// atomicMax, the sum as the fixed-point words of FgDacc (fg_internal.h; every cell is split exactly, the words are added as
// integers in registers, over the wave, over the workgroup, then with one atomic per word), the counts and bins as integer
// atomics.  So a result depends neither on the launch order nor on the other envs of the batch.
//
// Shape: 256 threads, one workgroup per (env, tile of FS_TILE cells): the headline field [64, 2, 256 x 128] is 64 x 8 = 512
// workgroups, two per CU.  16-byte loads when n is a multiple of the vector width and the field is 16-byte aligned (then every
// (env, channel) row starts aligned), scalar loads otherwise.  The histogram of a tile is built in LDS (32-bit counts, at most
// FS_TILE per bin) and its non-zero bins are flushed with 64-bit global atomics.
#include <float.h>

#include "fg_internal.h"

namespace {

constexpr int FS_TILE = 4096;          // cells per workgroup: 16 per thread
constexpr int FS_MAX_BINS = 4096;      // 16 KB of LDS counts
constexpr int FS_VEC = FG_F64 ? 2 : 4; // reals per 16-byte load

// per-env accumulators of one call (FG_FIELD_SUMMARY_WORK_BYTES each), initialised and consumed inside the call
struct alignas(64) FsWork {
    FgDacc sum;
    unsigned long long kmin, kmax, n_finite, n_bad;
    unsigned long long pad[4];
};
static_assert(sizeof(FsWork) == FG_FIELD_SUMMARY_WORK_BYTES, "workspace size of the header");

// doubles as unsigned keys with the same order (finite values and infinities; NaN never gets here)
__device__ __forceinline__ unsigned long long fs_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double fs_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

struct FsArgs {
    const fg_real* field;
    long long n;
    int channels, channel;     // channel < 0: magnitude over all channels
    FsWork* work;
    double lo, width;
    int nbins;
    unsigned long long* hist;  // [batch][nbins]
};

template <int VEC>
__device__ __forceinline__ void fs_load(const fg_real* p, double (&v)[VEC]) {
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

__global__ void k_fs_init(FsWork* __restrict__ w, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    acc_st(&w[b].sum, 0.0);
    w[b].sum.poison = 0ull;
    w[b].kmin = ~0ull; w[b].kmax = 0ull; w[b].n_finite = 0ull; w[b].n_bad = 0ull;
}

// moments [batch][3] = min, max, sum (NaN, NaN, 0 for an env without a finite cell); counts [batch][2] = finite, non-finite
__global__ void k_fs_finish(const FsWork* __restrict__ w, int batch, double* __restrict__ moments, long long* __restrict__ counts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const unsigned long long nf = w[b].n_finite;
    moments[3 * b + 0] = nf ? fs_unkey(w[b].kmin) : (double)NAN;
    moments[3 * b + 1] = nf ? fs_unkey(w[b].kmax) : (double)NAN;
    moments[3 * b + 2] = acc_ld(&w[b].sum);
    counts[2 * b + 0] = (long long)nf;
    counts[2 * b + 1] = (long long)w[b].n_bad;
}

template <int VEC, bool MAG, bool MOM, bool HIST>
__global__ __launch_bounds__(256) void k_field_summary(FsArgs a) {
    extern __shared__ unsigned int s_hist[];                 // HIST: nbins counts
    __shared__ long long s_k[4][FG_DACC_WORDS];
    __shared__ double s_mn[4], s_mx[4];
    __shared__ unsigned int s_nf[4], s_nb[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * FS_TILE;
    const long long t1 = (t0 + FS_TILE < a.n) ? t0 + FS_TILE : a.n;
    const fg_real* base = a.field + (size_t)b * (size_t)a.channels * (size_t)a.n;
    if (HIST) {
        for (int i = tid; i < a.nbins; i += 256) s_hist[i] = 0u;
        __syncthreads();
    }
    double mn = INFINITY, mx = -INFINITY;
    long long kw[FG_DACC_WORDS];
#pragma unroll
    for (int q = 0; q < FG_DACC_WORDS; ++q) kw[q] = 0;
    unsigned int nf = 0, nb = 0;
    const double top = (double)(a.nbins - 1);
    // (vector path: n % VEC == 0, so a group that starts below t1 ends at or below it)
    for (long long i = t0 + (long long)tid * VEC; i < t1; i += 256 * VEC) {
        double v[VEC];
        if (MAG) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = 0.0;
            for (int c = 0; c < a.channels; ++c) {           // ascending channel order, fp64
                double x[VEC];
                fs_load<VEC>(base + (size_t)c * (size_t)a.n + i, x);
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[j] += x[j] * x[j];
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = sqrt(v[j]);
        } else {
            fs_load<VEC>(base + (size_t)a.channel * (size_t)a.n + i, v);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double x = v[j];
            if (!(fabs(x) <= DBL_MAX)) { ++nb; continue; }   // NaN, Inf: counted, neither summed nor binned
            if (MOM) {
                ++nf;
                mn = fmin(mn, x); mx = fmax(mx, x);
                long long k[5];
                fg_dacc_split(x, k);
#pragma unroll
                for (int q = 0; q < FG_DACC_WORDS; ++q) kw[q] += k[q];
            }
            if (HIST) {
                double t = floor((x - a.lo) / a.width);      // IEEE subtraction and division: the host's fp64 expression
                t = t < 0.0 ? 0.0 : (t > top ? top : t);
                atomicAdd(&s_hist[(int)t], 1u);
            }
        }
    }
    if (MOM) {
        // wave, then workgroup; every combination is an integer sum or a min / max
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn = fmin(mn, __shfl_xor(mn, off, 64));
            mx = fmax(mx, __shfl_xor(mx, off, 64));
            nf += __shfl_xor(nf, off, 64);
            nb += __shfl_xor(nb, off, 64);
#pragma unroll
            for (int q = 0; q < FG_DACC_WORDS; ++q) kw[q] += __shfl_xor(kw[q], off, 64);
        }
        const int wave = tid >> 6;
        if ((tid & 63) == 0) {
            s_mn[wave] = mn; s_mx[wave] = mx; s_nf[wave] = nf; s_nb[wave] = nb;
#pragma unroll
            for (int q = 0; q < FG_DACC_WORDS; ++q) s_k[wave][q] = kw[q];
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) {
                mn = fmin(mn, s_mn[w]); mx = fmax(mx, s_mx[w]); nf += s_nf[w]; nb += s_nb[w];
#pragma unroll
                for (int q = 0; q < FG_DACC_WORDS; ++q) kw[q] += s_k[w][q];
            }
            FsWork* w = a.work + b;
            if (nf) {
                atomicMin(&w->kmin, fs_key(mn));
                atomicMax(&w->kmax, fs_key(mx));
                atomicAdd(&w->n_finite, (unsigned long long)nf);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (kw[q] != 0) atomicAdd(&w->sum.w[q], (unsigned long long)kw[q]);
#if FG_DACC_WORDS == 5
                if (kw[4] != 0) atomicAdd(&w->sum.w4, (unsigned long long)kw[4]);
#endif
            }
            if (nb) atomicAdd(&w->n_bad, (unsigned long long)nb);
        }
    }
    if (HIST) {
        __syncthreads();
        unsigned long long* h = a.hist + (size_t)b * (size_t)a.nbins;
        for (int i = tid; i < a.nbins; i += 256) {
            const unsigned int c = s_hist[i];
            if (c) atomicAdd(h + i, (unsigned long long)c);
        }
    }
}

template <int VEC, bool MAG>
void fs_launch(const FsArgs& a, bool mom, bool hist, dim3 grid, hipStream_t st) {
    const size_t lds = hist ? sizeof(unsigned int) * (size_t)a.nbins : 0;
    if (mom && hist) hipLaunchKernelGGL((k_field_summary<VEC, MAG, true, true>), grid, dim3(256), lds, st, a);
    else if (mom) hipLaunchKernelGGL((k_field_summary<VEC, MAG, true, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_field_summary<VEC, MAG, false, true>), grid, dim3(256), lds, st, a);
}

}  // namespace

extern "C" int fg_field_summary(const fg_real* field, int32_t batch, int32_t channels, int64_t n, int32_t channel, void* workspace,
                                double* moments, int64_t* counts, double lo, double width, int32_t nbins, uint64_t* hist,
                                void* stream) {
    const bool mom = moments != nullptr || counts != nullptr || workspace != nullptr;
    const bool his = hist != nullptr;
    FG_REQUIRE(field, FG_ERR_INVALID_ARG, "fg_field_summary: null field");
    FG_REQUIRE(mom || his, FG_ERR_INVALID_ARG, "fg_field_summary: null outputs (neither moments nor a histogram requested)");
    FG_REQUIRE(!mom || (moments && counts && workspace), FG_ERR_INVALID_ARG,
               "fg_field_summary: null pointer (the moments need workspace, moments and counts)");
    FG_REQUIRE(n > 0, FG_ERR_INVALID_ARG, "fg_field_summary: n must be positive");
    FG_REQUIRE(batch > 0 && batch <= 65535, FG_ERR_INVALID_ARG, "fg_field_summary: batch must be 1..65535");
    FG_REQUIRE(channels > 0, FG_ERR_INVALID_ARG, "fg_field_summary: channels must be positive");
    FG_REQUIRE(channel >= -1 && channel < channels, FG_ERR_INVALID_ARG, "fg_field_summary: channel out of range (-1 = magnitude)");
    FG_REQUIRE((n + FS_TILE - 1) / FS_TILE <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_field_summary: n too large for one launch");
    if (his) {
        FG_REQUIRE(nbins >= 1 && nbins <= FS_MAX_BINS, FG_ERR_INVALID_ARG, "fg_field_summary: nbins must be 1..4096");
        FG_REQUIRE(width > 0.0 && width <= DBL_MAX && fabs(lo) <= DBL_MAX, FG_ERR_INVALID_ARG,
                   "fg_field_summary: width must be positive and finite, lo finite");
    }
    hipStream_t st = (hipStream_t)stream;
    FsArgs a;
    a.field = field; a.n = (long long)n; a.channels = channels; a.channel = channel;
    a.work = (FsWork*)workspace; a.lo = lo; a.width = width; a.nbins = his ? nbins : 1; a.hist = (unsigned long long*)hist;
    const dim3 grid((unsigned)((n + FS_TILE - 1) / FS_TILE), (unsigned)batch);
    const int tiny = (batch + 63) / 64;
    if (mom) hipLaunchKernelGGL(k_fs_init, dim3(tiny), dim3(64), 0, st, a.work, batch);
    const bool vec = (n % FS_VEC == 0) && ((uintptr_t)field % 16 == 0);
    const bool mag = channel < 0;
    if (vec) { if (mag) fs_launch<FS_VEC, true>(a, mom, his, grid, st); else fs_launch<FS_VEC, false>(a, mom, his, grid, st); }
    else     { if (mag) fs_launch<1, true>(a, mom, his, grid, st); else fs_launch<1, false>(a, mom, his, grid, st); }
    if (mom) hipLaunchKernelGGL(k_fs_finish, dim3(tiny), dim3(64), 0, st, (const FsWork*)a.work, batch, moments, (long long*)counts);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
