// Online Welch power and cross spectra of per-env scalar signals (SignalSpectra, simulation/signal_spectra.py): drag, lift, probe
// values, wall stresses -- a handful of numbers per env and sim step, of which the question is "at which frequency".
//
// One call is one sample of a batch of B envs and ONE launch; the host reads nothing back and decides nothing per env:
//   append   the S = sum n_i values of an env, read in place from up to 8 source arrays [B, n_i], go into the env's ring
//            ring [B, S, L] at fill[b] % L, and fill[b] -- the samples since the env last (re)started -- is incremented
//   due      a segment of an env is due when fill >= L and (fill - L) % hop == 0, hop = L - noverlap: decided here, per env, because
//            envs are out of phase with each other after per-env restarts.  A workgroup with nothing due ends behind the append.
//   segment  a job is one signal (its auto spectrum) or one listed pair (its cross spectrum): the L ring values of a signal in time
//            order, the sums of the detrend in fp64 (0 none, 1 the mean, 2 the least-squares line), times window[t] (a device table
//            of doubles made by the host), rounded to fg_real once, and a length-L Stockham autosort FFT in the wave's LDS buffers
//            (fg_stockham.h; twiddles from sincospi of the exact argument in fp64, rounded once per workgroup).  |X_s|^2 and
//            conj(X_a) X_b (SciPy's csd convention) are evaluated in fp64 and ADDED to power [B, S, L/2+1] and
//            cross [B, n_pairs, L/2+1, 2]; `last` [B, S, L/2+1], when given, is overwritten with this segment's |X_s|^2;
//            segments [B] counts.  DC and Nyquist are kept.
//
// Every signal is transformed on its own, with a zero imaginary part.  Packing two real signals into one complex transform would
// halve the FFT work, but the rounding of either spectrum would then depend on the other signal: a non-finite sample of one would
// change the bits of its partner, and a signal's numbers would depend on which pairs are listed.  Here a signal's spectrum is a pure
// function of its own L samples, the window and the detrend; a pair job repeats the two transforms of its signals (the same code on
// the same data, hence the same bits as their auto jobs: the cross spectrum of a signal with itself is its power, with a zero
// imaginary part).  A segment is S + n_pairs <= 128 jobs of O(L log L) once every hop samples: small against the launch itself.
//
// Ownership: one workgroup of four waves per env.  The first S threads append; after a workgroup barrier the waves take the jobs
// round robin, each in its own three LDS buffers of L complex (two for a transform, a third so that a pair job holds its first
// spectrum while the second is made).  Element (s, k) of power / last and (p, k) of cross belong to one lane of the wave that has the
// job: no atomics, and an env's numbers depend on nothing but its own samples and the spec -- not on B, the row, or which other envs
// had a segment due.  LDS: (1 + 3 W) L complex for W working waves, W = the most of 4 that fit 160 KB; L = 16 .. 4096 (fp32) /
// 16 .. 2048 (fp64).
//
// A non-finite value among the L samples of a signal makes that signal's |X|^2 of the segment, hence its power from then on, and
// the cross spectra of its pairs NaN, by rule and not by luck; nothing else changes by a bit.
#include <float.h>

#include <mutex>

#include "fg_stockham.h"

namespace {

constexpr int SS_MAX_SOURCES = 8;
constexpr int SS_MAX_SIGNALS = 64;
constexpr int SS_MAX_PAIRS = 64;
constexpr int SS_WAVES = 4;
constexpr int SS_MIN_L = 16;
constexpr int SS_LDS_LIMIT = 160 * 1024;          // what a workgroup may declare on gfx950

struct SsArgs {
    const fg_real* src[SS_MAX_SOURCES];
    long long bstride[SS_MAX_SOURCES];
    unsigned char sig_src[SS_MAX_SIGNALS], sig_col[SS_MAX_SIGNALS];     // signal s is column sig_col[s] of source sig_src[s]
    unsigned char pair_a[SS_MAX_PAIRS], pair_b[SS_MAX_PAIRS];
    int S, n_pairs, L, lnL, hop, detrend, waves;
    const double* window;
    fg_real* ring;
    long long* fill;
    double* power;
    double* cross;
    long long* segments;
    double* last;
};

// what the kernel declares for a segment of L with `waves` working waves: twiddles and three buffers per wave
inline long long ss_lds_bytes(int L, int waves) { return (1LL + 3LL * waves) * L * (long long)sizeof(ps_c); }
inline int ss_waves(int L) {
    int w = SS_WAVES;
    while (w > 0 && ss_lds_bytes(L, w) > SS_LDS_LIMIT) --w;
    return w;
}

__device__ __forceinline__ double ss_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The spectrum of one signal of the segment that starts at ring position `start`: detrended in fp64, windowed, rounded to fg_real,
// transformed in (x, y); returns the buffer that holds the L modes.  bad: a non-finite sample among the L.
__device__ __forceinline__ ps_c* ss_transform(const SsArgs& a, const fg_real* __restrict__ sig, int start, ps_c* x, ps_c* y,
                                              const ps_c* __restrict__ tw, int lane, bool& bad) {
    const int L = a.L;
    const double mid = 0.5 * (double)(L - 1);
    double s0 = 0.0, s1 = 0.0;
    int nf = 0;
    if (a.detrend != 0) {
        for (int t = lane; t < L; t += 64) {
            const double v = (double)sig[(start + t) & (L - 1)];
            s0 += v;
            s1 += ((double)t - mid) * v;
        }
        s0 = ss_wave_sum(s0);
        s1 = ss_wave_sum(s1);
    }
    const double mean = a.detrend != 0 ? s0 / (double)L : 0.0;
    // sum (t - mid)^2 = L (L^2 - 1) / 12
    const double slope = a.detrend == 2 ? s1 / ((double)L * ((double)L * (double)L - 1.0) / 12.0) : 0.0;
    for (int t = lane; t < L; t += 64) {
        const double v = (double)sig[(start + t) & (L - 1)];
        nf |= !(fabs(v) <= DBL_MAX);
        const double d = v - (mean + slope * ((double)t - mid));
        x[t] = ps_make((fg_real)(d * a.window[t]), (fg_real)0);
    }
    bad = __any(nf) != 0;
    ps_wave_sync();
    return ps_stockham(x, y, tw, a.lnL, 1, L, lane);
}

__global__ __launch_bounds__(256) void k_signal_spectra(SsArgs a) {
    extern __shared__ __align__(16) unsigned char ss_lds[];
    ps_c* tw = reinterpret_cast<ps_c*>(ss_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, L = a.L, S = a.S;
    fg_real* ring = a.ring + (long long)b * S * L;

    // ---- append: every thread reads the counter before thread 0 moves it
    const long long f = a.fill[b];
    const int pos = (int)(f & (long long)(L - 1));
    if (tid < S) {
        const int i = a.sig_src[tid];
        ring[(long long)tid * L + pos] = a.src[i][(long long)b * a.bstride[i] + a.sig_col[tid]];
    }
    __syncthreads();
    const long long f1 = f + 1;
    if (tid == 0) a.fill[b] = f1;
    if (f1 < L || (f1 - L) % a.hop != 0) return;             // (uniform over the workgroup) no segment of this env is due

    for (int i = tid; i < L; i += 256) {
        double s, c;
        sincospi(2.0 * (double)i / (double)L, &s, &c);
        tw[i] = ps_make((fg_real)c, (fg_real)s);
    }
    __syncthreads();

    if (wave < a.waves) {
        ps_c* w0 = tw + L + (long long)wave * 3 * L;
        ps_c* w1 = w0 + L;
        ps_c* w2 = w1 + L;
        const int start = (pos + 1) & (L - 1), half = L / 2 + 1;
        for (int job = wave; job < S + a.n_pairs; job += a.waves) {
            if (job < S) {
                bool bad;
                const ps_c* X = ss_transform(a, ring + (long long)job * L, start, w0, w1, tw, lane, bad);
                double* gp = a.power + ((long long)b * S + job) * half;
                double* gl = a.last ? a.last + ((long long)b * S + job) * half : nullptr;
                for (int k = lane; k < half; k += 64) {
                    const double re = (double)X[k].x, im = (double)X[k].y;
                    const double p = bad ? (double)NAN : re * re + im * im;
                    gp[k] += p;
                    if (gl) gl[k] = p;
                }
            } else {
                const int p = job - S;
                bool bad_a, bad_b;
                ps_c* XA = ss_transform(a, ring + (long long)a.pair_a[p] * L, start, w0, w1, tw, lane, bad_a);
                const ps_c* XB = ss_transform(a, ring + (long long)a.pair_b[p] * L, start, XA == w0 ? w1 : w0, w2, tw, lane, bad_b);
                const bool bad = bad_a || bad_b;
                double* gc = a.cross + (((long long)b * a.n_pairs + p) * half) * 2;
                for (int k = lane; k < half; k += 64) {
                    const double ar = (double)XA[k].x, ai = (double)XA[k].y, br = (double)XB[k].x, bi = (double)XB[k].y;
                    gc[2 * k] += bad ? (double)NAN : ar * br + ai * bi;
                    gc[2 * k + 1] += bad ? (double)NAN : ar * bi - ai * br;
                }
            }
            ps_wave_sync();      // the buffers are staged again by the next job
        }
    }
    if (tid == 0) a.segments[b] += 1;
}

// kernels that declare more than 64 KB of dynamic LDS opt in once per device
bool ss_opt_in() {
    static std::mutex mu;
    static int state[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return false; }
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
        state[dev] = 1;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_signal_spectra), hipFuncAttributeMaxDynamicSharedMemorySize, SS_LDS_LIMIT) !=
            hipSuccess) {
            (void)hipGetLastError();
            state[dev] = -1;
        }
    }
    return state[dev] == 1;
}

}  // namespace

extern "C" int fg_signal_spectra(const fg_real* const* sources, const int64_t* batch_stride, const int32_t* widths, int32_t n_sources,
                                 int32_t batch, int32_t segment, int32_t noverlap, int32_t detrend, const double* window,
                                 const int32_t* pairs, int32_t n_pairs, fg_real* ring, int64_t* fill, double* power, double* cross,
                                 int64_t* segments, double* last, void* stream) {
    FG_REQUIRE(sources && batch_stride && widths, FG_ERR_INVALID_ARG, "fg_signal_spectra: null source, stride or width table");
    FG_REQUIRE(window && ring && fill && power && segments, FG_ERR_INVALID_ARG,
               "fg_signal_spectra: null window, ring, fill, power or segments");
    FG_REQUIRE(n_sources >= 1 && n_sources <= SS_MAX_SOURCES, FG_ERR_INVALID_ARG, "fg_signal_spectra: n_sources must be 1..8");
    FG_REQUIRE(n_pairs >= 0 && n_pairs <= SS_MAX_PAIRS, FG_ERR_INVALID_ARG, "fg_signal_spectra: n_pairs must be 0..64");
    FG_REQUIRE(n_pairs == 0 || (pairs && cross), FG_ERR_INVALID_ARG, "fg_signal_spectra: null pair table or cross with n_pairs > 0");
    FG_REQUIRE(batch > 0, FG_ERR_INVALID_ARG, "fg_signal_spectra: batch must be positive");
    FG_REQUIRE(detrend >= 0 && detrend <= 2, FG_ERR_INVALID_ARG, "fg_signal_spectra: detrend must be 0 (none), 1 (constant) or 2 (linear)");
    SsArgs a;
    int S = 0;
    for (int i = 0; i < SS_MAX_SOURCES; ++i) { a.src[i] = nullptr; a.bstride[i] = 0; }
    for (int s = 0; s < SS_MAX_SIGNALS; ++s) a.sig_src[s] = a.sig_col[s] = 0;
    for (int i = 0; i < n_sources; ++i) {
        FG_REQUIRE(sources[i], FG_ERR_INVALID_ARG, "fg_signal_spectra: null source pointer");
        FG_REQUIRE(widths[i] >= 1 && widths[i] <= SS_MAX_SIGNALS && S + widths[i] <= SS_MAX_SIGNALS, FG_ERR_INVALID_ARG,
                   "fg_signal_spectra: the widths must be positive and sum to 1..64 signals");
        FG_REQUIRE(batch_stride[i] >= widths[i], FG_ERR_INVALID_ARG, "fg_signal_spectra: batch stride smaller than the source's width");
        a.src[i] = sources[i]; a.bstride[i] = batch_stride[i];
        for (int c = 0; c < widths[i]; ++c, ++S) { a.sig_src[S] = (unsigned char)i; a.sig_col[S] = (unsigned char)c; }
    }
    for (int p = 0; p < SS_MAX_PAIRS; ++p) {
        a.pair_a[p] = a.pair_b[p] = 0;
        if (p >= n_pairs) continue;
        FG_REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < S && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < S, FG_ERR_INVALID_ARG,
                   "fg_signal_spectra: a pair index outside [0, S)");
        a.pair_a[p] = (unsigned char)pairs[2 * p]; a.pair_b[p] = (unsigned char)pairs[2 * p + 1];
    }
    FG_REQUIRE(segment >= 1 && noverlap >= 0 && noverlap < segment, FG_ERR_INVALID_ARG, "fg_signal_spectra: noverlap must lie in [0, segment)");
    FG_REQUIRE(segment >= SS_MIN_L && (segment & (segment - 1)) == 0, FG_ERR_UNSUPPORTED,
               "fg_signal_spectra: segment must be a power of two, at least 16");
    const int waves = segment <= SS_LDS_LIMIT ? ss_waves(segment) : 0;
    FG_REQUIRE(waves >= 1, FG_ERR_UNSUPPORTED,
               FG_F64 ? "fg_signal_spectra: twiddles and three buffers of `segment` complex doubles must fit in 160 KB of LDS (segment <= 2048)"
                      : "fg_signal_spectra: twiddles and three buffers of `segment` complex floats must fit in 160 KB of LDS (segment <= 4096)");
    int ln = 0;
    while ((1 << ln) < segment) ++ln;
    a.S = S; a.n_pairs = n_pairs; a.L = segment; a.lnL = ln; a.hop = segment - noverlap; a.detrend = detrend; a.waves = waves;
    a.window = window; a.ring = ring; a.fill = reinterpret_cast<long long*>(fill); a.power = power; a.cross = cross;
    a.segments = reinterpret_cast<long long*>(segments); a.last = last;
    FG_REQUIRE(ss_opt_in(), FG_ERR_HIP, "fg_signal_spectra: the device refused 160 KB of LDS per workgroup");
    hipLaunchKernelGGL(k_signal_spectra, dim3((unsigned)batch), dim3(256), (size_t)ss_lds_bytes(segment, waves), (hipStream_t)stream, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
