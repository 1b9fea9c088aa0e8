// Online wavenumber spectra of wall-parallel planes (PlaneSpectra, simulation/plane_spectra.py): for every slab (env, channel k,
// listed plane j) the unnormalised DFT of the real plane [nz, nx] over (z, x) -- over x alone for 2-D fields, nz = 1 -- and the
// running sums of |u^| and |u^|^2 of the modes kz < max(nz / 2, 1), kx < nx / 2.
//
// The reference keeps these with PSDOnline_Torch (pict/data/online_statistics.py:269-416; fed by VelocityStats.record_vel_stats,
// TCF_tools.py:445-459, 1491-1500): an index_select copy of the planes, a full complex fftn in HBM, an abs, a slice, a mean and a
// merge, all of it twice for the mirrored planes.  Here one sample of a batch is ONE launch that reads every selected plane once
// and reads and writes the accumulators once.
//
// Ownership and order: one workgroup of four waves owns a slab and holds its nz x nx/2 half spectrum in LDS.
//   x pass   a wave takes batches of row PAIRS (z, z + 1): the two real rows are the real and imaginary part of one complex row,
//            transformed by a Stockham autosort FFT (radix 4, then one radix 2) in the wave's own two work buffers and split into
//            the two rows' spectra, of which only kx < nx / 2 is kept (real input; the Nyquist column is not recorded).  As many
//            pairs go into one batch as the work buffer holds, so that short rows still fill the 64 lanes.
//   z pass   a wave copies batches of columns kx out of the slab into its work buffers, transforms them the same way and writes
//            kz < nz / 2 back to the columns it took, which no other wave touches.
//   sums     the 256 threads walk the kept modes in memory order and add |u^| and |u^|^2 (evaluated in fp64) to the accumulators:
//            one thread per element, no atomics.  A slab's result depends on nothing but its cells and the extents.
// LDS layout: slab rows are nx / 2 + 1 complex apart.  The z pass reads and writes the slab along z with consecutive lanes on
// consecutive z; at a row pitch of nx / 2 complex (a power of two, >= one 256-byte bank row from nx = 64 on) every lane of a group
// would hit the same banks, with one complex of padding consecutive z are 2 (fp32) / 4 (fp64) banks apart and the 32 / 16 lanes
// of an 8- / 16-byte access group cover the 64 banks once.
// Twiddles: (cos, sin)(2 pi k / max(nx, nz)) from sincospi of the exact argument 2 k / max(nx, nz) in fp64, rounded to fg_real once
// per workgroup into LDS; a shorter axis reads the table with a stride.
#include <float.h>

#include <mutex>

#include "fg_rowstat.h"
#include "fg_stockham.h"

namespace {

namespace rs = fg_rowstat;

constexpr int PS_MAX_K = 5;
constexpr int PS_MAX_PLANES = 32;
constexpr int PS_WAVES = 4;
constexpr int PS_LDS_LIMIT = 160 * 1024;          // what a workgroup may declare on gfx950
constexpr fg_real PS_REAL_MAX = FG_F64 ? (fg_real)DBL_MAX : (fg_real)FLT_MAX;
constexpr int PS_WORK_MIN =2048 / (int)sizeof(ps_c);   // a work buffer holds at least 2 KB: 256 (fp32) / 128 (fp64) complex

struct PsArgs {
    rs::ChannelTable<PS_MAX_K> t;         // loads and their checks: fg_rowstat.h
    int planes[PS_MAX_PLANES];
    long long zstride;                    // ny * nx
    int K, n_planes, nz, nx, lnz, lnx;    // ln = log2
    int pitch, work, nmax, vec;           // slab row pitch and work buffer length in complex; max(nx, nz); 16-byte loads
    double* amp;
    double* power;
};

// what the kernel declares for extents (nz, nx): twiddles, slab, two work buffers per wave, the non-finite flag
inline long long ps_work(int nz, int nx) { const int m = nx > nz ? nx : nz; return m > PS_WORK_MIN ? m : PS_WORK_MIN; }
inline long long ps_lds_bytes(int nz, int nx) {
    const long long nmax = nx > nz ? nx : nz;
    return (nmax + (long long)nz * (nx / 2 + 1) + 2 * PS_WAVES * ps_work(nz, nx)) * (long long)sizeof(ps_c) + 16;
}

// VEC consecutive reals of the rows at pa and pb (pb == nullptr: a 2-D field, the imaginary row is 0) as VEC complex at dst
template <int VEC>
__device__ __forceinline__ bool ps_stage(const fg_real* pa, const fg_real* pb, ps_c* dst) {
    fg_real va[VEC], vb[VEC];
    rs::load<VEC>(pa, va);
#pragma unroll
    for (int e = 0; e < VEC; ++e) vb[e] = (fg_real)0;
    if (pb) rs::load<VEC>(pb, vb);
    bool bad = false;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        dst[e] = ps_make(va[e], vb[e]);
        bad = bad || !(FG_FABS(va[e]) <= PS_REAL_MAX) || !(FG_FABS(vb[e]) <= PS_REAL_MAX);
    }
    return bad;
}

// one kernel for both load widths (a.vec is uniform): the arithmetic, hence the bits, cannot depend on how the rows were loaded
__global__ __launch_bounds__(256) void k_plane_spectra(PsArgs a) {
    extern __shared__ __align__(16) unsigned char ps_lds[];
    ps_c* tw = reinterpret_cast<ps_c*>(ps_lds);
    ps_c* slab = tw + a.nmax;
    ps_c* work = slab + a.nz * a.pitch;
    int* s_bad = reinterpret_cast<int*>(work + 2 * PS_WAVES * a.work);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sid = blockIdx.x;
    const int j = sid % a.n_planes, k = (sid / a.n_planes) % a.K, b = sid / (a.n_planes * a.K);
    const fg_real* base = a.t.ch[k] + (long long)b * a.t.bstride[k] + (long long)a.planes[j] * a.nx;
    const int nz = a.nz, nx = a.nx, hx = nx >> 1, lhx = a.lnx - 1, pitch = a.pitch;
    ps_c* x = work + wave * 2 * a.work;
    ps_c* y = x + a.work;

    for (int i = tid; i < a.nmax; i += 256) {
        double s, c;
        sincospi(2.0 * (double)i / (double)a.nmax, &s, &c);
        tw[i] = ps_make((fg_real)c, (fg_real)s);
    }
    if (tid == 0) *s_bad = 0;
    __syncthreads();

    // ---- x pass: row pairs (2 q, 2 q + 1), nb pairs per batch
    {
        const int npairs = nz > 1 ? nz >> 1 : 1;
        int nb = a.work >> a.lnx;
        nb = nb < npairs ? nb : npairs;
        const int lvec = a.vec ? (rs::VEC == 4 ? 2 : 1) : 0, lnxv = a.lnx - lvec;
        const int tws = a.nmax >> a.lnx;
        bool bad = false;
        for (int q0 = wave * nb; q0 < npairs; q0 += PS_WAVES * nb) {
            for (int i = lane; i < (nb << lnxv); i += 64) {
                const int s = i >> lnxv, xe = (i & ((1 << lnxv) - 1)) << lvec;
                const fg_real* pa = base + (long long)(2 * (q0 + s)) * a.zstride + xe;
                const fg_real* pb = nz > 1 ? pa + a.zstride : nullptr;
                ps_c* dst = x + (s << a.lnx) + xe;
                bad = (a.vec ? ps_stage<rs::VEC>(pa, pb, dst) : ps_stage<1>(pa, pb, dst)) || bad;
            }
            ps_wave_sync();
            const ps_c* X = ps_stockham(x, y, tw, a.lnx, tws, nb << a.lnx, lane);
            // the spectrum of z = a + i b split into those of the rows:  A = (Z_k + conj Z_{n-k}) / 2,  B = (Z_k - conj Z_{n-k}) / 2i
            for (int i = lane; i < (nb << lhx); i += 64) {
                const int s = i >> lhx, kx = i & (hx - 1);
                const ps_c Z = X[(s << a.lnx) + kx], M = X[(s << a.lnx) + ((nx - kx) & (nx - 1))];
                ps_c* row = slab + (2 * (q0 + s)) * pitch + kx;
                row[0] = ps_make((fg_real)0.5 * (Z.x + M.x), (fg_real)0.5 * (Z.y - M.y));
                if (nz > 1) row[pitch] = ps_make((fg_real)0.5 * (Z.y + M.y), (fg_real)-0.5 * (Z.x - M.x));
            }
            ps_wave_sync();      // the work buffers are staged again by the next batch
        }
        if (bad) *s_bad = 1;
    }
    __syncthreads();

    // ---- z pass: columns kx < nx / 2, nbc columns per batch; consecutive lanes on consecutive z (see the layout note above)
    if (nz > 1) {
        const int hz = nz >> 1, lhz = a.lnz - 1;
        int nbc = a.work >> a.lnz;
        nbc = nbc < hx ? nbc : hx;
        const int tws = a.nmax >> a.lnz;
        for (int c0 = wave * nbc; c0 < hx; c0 += PS_WAVES * nbc) {
            for (int i = lane; i < (nbc << a.lnz); i += 64) x[i] = slab[(i & (nz - 1)) * pitch + c0 + (i >> a.lnz)];
            ps_wave_sync();
            const ps_c* X = ps_stockham(x, y, tw, a.lnz, tws, nbc << a.lnz, lane);
            for (int i = lane; i < (nbc << lhz); i += 64) {
                const int c = i >> lhz, kz = i & (hz - 1);
                slab[kz * pitch + c0 + c] = X[(c << a.lnz) + kz];
            }
            ps_wave_sync();
        }
        __syncthreads();
    }

    // ---- sums: element (kz, kx) of this slab's accumulators belongs to one thread
    const int kept = (nz > 1 ? nz >> 1 : 1) << lhx;
    const bool poisoned = *s_bad != 0;       // a non-finite cell anywhere in the slab: every mode of it is NaN, by rule and not by luck
    double* ga = a.amp + (long long)sid * kept;
    double* gp = a.power + (long long)sid * kept;
    for (int i = tid; i < kept; i += 256) {
        const ps_c v = slab[(i >> lhx) * pitch + (i & (hx - 1))];
        const double re = (double)v.x, im = (double)v.y;
        double p = re * re + im * im, m = sqrt(p);
        if (poisoned) p = m = (double)NAN;
        ga[i] += m;
        gp[i] += p;
    }
}

// kernels that declare more than 64 KB of dynamic LDS opt in once per device
bool ps_opt_in() {
    static std::mutex mu;
    static int state[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return false; }
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
        state[dev] = 1;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_plane_spectra), hipFuncAttributeMaxDynamicSharedMemorySize, PS_LDS_LIMIT) !=
            hipSuccess) {
            (void)hipGetLastError();
            state[dev] = -1;
        }
    }
    return state[dev] == 1;
}

inline int ps_log2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

}  // namespace

extern "C" int fg_plane_spectra(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz,
                                int32_t ny, int32_t nx, const int32_t* planes, int32_t n_planes, double* amp, double* power,
                                void* stream) {
    FG_REQUIRE(channels && batch_stride && planes, FG_ERR_INVALID_ARG, "fg_plane_spectra: null channel, stride or plane table");
    FG_REQUIRE(amp && power, FG_ERR_INVALID_ARG, "fg_plane_spectra: null accumulator (amp, power)");
    FG_REQUIRE(K >= 1 && K <= PS_MAX_K, FG_ERR_INVALID_ARG, "fg_plane_spectra: K must be 1..5");
    FG_REQUIRE(n_planes >= 1 && n_planes <= PS_MAX_PLANES, FG_ERR_INVALID_ARG, "fg_plane_spectra: n_planes must be 1..32");
    FG_REQUIRE(batch > 0 && nz > 0 && ny > 0 && nx > 0, FG_ERR_INVALID_ARG, "fg_plane_spectra: batch, nz, ny, nx must be positive");
    FG_REQUIRE((long long)batch * K * n_planes <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_plane_spectra: batch * K * n_planes too large for one launch");
    PsArgs a;
    for (int j = 0; j < PS_MAX_PLANES; ++j) {
        a.planes[j] = 0;
        if (j >= n_planes) continue;
        FG_REQUIRE(planes[j] >= 0 && planes[j] < ny, FG_ERR_INVALID_ARG, "fg_plane_spectra: plane index outside [0, ny)");
        a.planes[j] = planes[j];
    }
    bool vec;
    const int rc = rs::fill(a.t, vec, "fg_plane_spectra", "channel", channels, batch_stride, K, nz, ny, nx);
    if (rc != FG_OK) return rc;
    FG_REQUIRE(nx >= 8 && nx <= 512 && (nx & (nx - 1)) == 0, FG_ERR_UNSUPPORTED, "fg_plane_spectra: nx must be a power of two in 8..512");
    FG_REQUIRE(nz == 1 || (nz >= 4 && nz <= 256 && (nz & (nz - 1)) == 0), FG_ERR_UNSUPPORTED,
               "fg_plane_spectra: nz must be 1 or a power of two in 4..256");
    const long long lds = ps_lds_bytes(nz, nx);
    FG_REQUIRE(lds <= PS_LDS_LIMIT, FG_ERR_UNSUPPORTED,
               FG_F64 ? "fg_plane_spectra: the slab nz x (nx / 2 + 1) complex doubles with its work buffers must fit in 160 KB of LDS"
                      : "fg_plane_spectra: the slab nz x (nx / 2 + 1) complex floats with its work buffers must fit in 160 KB of LDS");
    a.zstride = (long long)ny * nx;
    a.K = K; a.n_planes = n_planes; a.nz = nz; a.nx = nx; a.lnz = ps_log2(nz); a.lnx = ps_log2(nx);
    a.pitch = nx / 2 + 1; a.work = (int)ps_work(nz, nx); a.nmax = nx > nz ? nx : nz; a.vec = vec ? 1 : 0;
    a.amp = amp; a.power = power;
    FG_REQUIRE(ps_opt_in(), FG_ERR_HIP, "fg_plane_spectra: the device refused 160 KB of LDS per workgroup");
    hipLaunchKernelGGL(k_plane_spectra, dim3((unsigned)(batch * K * n_planes)), dim3(256), (size_t)lds, (hipStream_t)stream, a);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
