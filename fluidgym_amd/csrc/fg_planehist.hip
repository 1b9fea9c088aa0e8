// Online PDFs and joint PDFs of wall-parallel planes (PlaneHistograms, simulation/plane_hist.py): for every listed row (env, y) the
// histogram of K channels over the homogeneous directions (z, x) and the joint histograms of chosen channel pairs, added to running
// 64-bit counters on the device.  The reference has no counterpart: it records moments and transforms of the planes only.
//
// Bin rule, in fg_real, two separately rounded operations (this file is compiled with -ffp-contract=off):
//   t = (v - lo[r][k]) * scale[r][k]
//   slot = bins + 2 if v is NaN;  0 if !(t >= 0);  bins + 1 if t >= bins;  1 + (int)t otherwise
// t is compared as a real before the conversion, so no value can overflow the cast.  A pair (a, b) takes the coarsened indices
// (slot - 1) / (bins / joint_bins) of its two channels when both slots are in 1..bins and the slab's last element otherwise.
//
// One sample of a batch is ONE launch per HG_ROW_CHUNK listed rows (the row table travels in the kernel arguments).  Ownership and
// loads are those of fg_rowstat.h: one 256-thread workgroup per row whose plane has more than 1024 cells, one wave of a four-wave
// workgroup per smaller row.  The sample's histograms live in LDS as 32-bit counters (a plane has at most 2^30 cells): zeroed,
// filled with no-return LDS integer atomics, then every non-zero counter is added to its 64-bit global counter by plain loads and
// stores -- a row has one owner per launch and launches are stream-ordered, so no global atomic exists and a zero bin costs no
// global access.  The small-plane form gives every wave its own quarter of the workgroup's LDS and is otherwise the same code; its
// waves never meet at a barrier (LDS operations of one wave complete in order).
//
// LDS rule: words = K (bins + 3) + n_pairs (joint_bins^2 + 1) 32-bit counters per row; 4 words bytes (16 words in the small-plane
// form: four rows per workgroup) must not exceed 160 KB.  K = 5, bins = 256, n_pairs = 3 fits with joint_bins = 64 in the workgroup
// form (54,344 B) and with joint_bins = 32 in the small-plane form (69,920 B).
#include <mutex>

#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

constexpr int HG_MAX_K = 5;
constexpr int HG_MAX_PAIRS = 6;
constexpr int HG_MAX_BINS = 256;
constexpr int HG_MAX_JOINT_BINS = 64;
constexpr int HG_ROW_CHUNK = 256;                  // listed rows per launch: 1 KB of kernel arguments
constexpr int HG_LDS_LIMIT = 160 * 1024;

struct HgArgs {
    rs::ChannelTable<HG_MAX_K> t;
    long long zstride, rows;             // ny_field * nx; batch * (listed rows of this launch)
    int nz, ny, nx;                      // ny: the listed rows of this launch -- what FG_ROWSTAT_OWN_ROW divides by; its `y` indexes `row_of`
    int row0, n_rows;                    // first listed row of this launch, all listed rows
    int bins, n_pairs, joint_bins, jmul; // jmul: (s * jmul) >> 16 == s / (bins / joint_bins) for every s < 256
    int words;                           // LDS counters per row
    const fg_real* lo;
    const fg_real* scale;
    unsigned long long* counts;
    unsigned long long* joint;
    int row_of[HG_ROW_CHUNK];
    unsigned char pair[HG_MAX_PAIRS][2];
};

// the bin rule without a branch: t clamped to [0, bins] before the conversion (exact: a comparison and a selection), so that t >= bins
// lands on bins + 1 by itself and no value can overflow the cast
__device__ __forceinline__ int hg_slot(fg_real v, fg_real lo, fg_real scale, int bins) {
    const fg_real t = (v - lo) * scale, top = (fg_real)bins;
    fg_real c = t < top ? t : top;
    c = c > (fg_real)0 ? c : (fg_real)0;
    int s = 1 + (int)c;
    s = t >= (fg_real)0 ? s : 0;
    return v != v ? bins + 2 : s;
}

// slot[k] - 1 for a k known only at run time: masks, so that the slots stay in registers (an indexed array goes to scratch)
template <int K>
__device__ __forceinline__ int hg_pick(const int (&slot)[K], int k) {
    int s = 0;
#pragma unroll
    for (int q = 0; q < K; ++q) s |= slot[q] & (k == q ? -1 : 0);
    return s - 1;
}

__device__ __forceinline__ void hg_count(unsigned* p) {
    (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the LDS writes before this point are visible to the reads after it: to the workgroup, or (WAVE) to the wave that owns the quarter
template <bool WAVE>
__device__ __forceinline__ void hg_sync() {
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <int K, int VEC, bool WAVE>
__global__ __launch_bounds__(256) void k_plane_histogram(HgArgs a) {
    extern __shared__ unsigned s_hist[];
    const int tid = threadIdx.x;
    FG_ROWSTAT_OWN_ROW(a, VEC, WAVE, tid);                   // y: index into this launch's listed rows
    unsigned* h = s_hist + (WAVE ? (tid >> 6) * a.words : 0);
    for (int i = t0; i < a.words; i += step) h[i] = 0u;
    hg_sync<WAVE>();

    const int r = a.row0 + y, slots = a.bins + 3, jslab = a.joint_bins * a.joint_bins + 1;
    const fg_real* base[K];
    fg_real lo[K], sc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        base[k] = a.t.ch[k] + (long long)b * a.t.bstride[k] + (long long)a.row_of[y] * a.nx;
        lo[k] = a.lo[(long long)r * K + k];
        sc[k] = a.scale[(long long)r * K + k];
    }
    unsigned* hj = h + K * slots;
    for (int i = t0; i < items; i += step) {
        const long long off = rs::item_offset<VEC>(i, nxv, a.zstride);
        fg_real v[K][VEC];
#pragma unroll
        for (int k = 0; k < K; ++k) rs::load<VEC>(base[k] + off, v[k]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            int slot[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                slot[k] = hg_slot(v[k][j], lo[k], sc[k], a.bins);
                hg_count(h + k * slots + slot[k]);
            }
            for (int p = 0; p < a.n_pairs; ++p) {
                const int sa = hg_pick<K>(slot, a.pair[p][0]), sb = hg_pick<K>(slot, a.pair[p][1]);
                const bool in = (unsigned)sa < (unsigned)a.bins && (unsigned)sb < (unsigned)a.bins;
                const int cell = in ? ((sa * a.jmul) >> 16) * a.joint_bins + ((sb * a.jmul) >> 16) : jslab - 1;
                hg_count(hj + p * jslab + cell);
            }
        }
    }
    hg_sync<WAVE>();

    const long long slab = (long long)b * a.n_rows + r;
    unsigned long long* gc = a.counts + slab * (K * slots);
    for (int i = t0; i < K * slots; i += step) {
        const unsigned c = h[i];
        if (c) gc[i] += c;
    }
    if (a.n_pairs > 0) {
        unsigned long long* gj = a.joint + slab * ((long long)a.n_pairs * jslab);
        for (int i = t0; i < a.n_pairs * jslab; i += step) {
            const unsigned c = hj[i];
            if (c) gj[i] += c;
        }
    }
}

// every instance may declare up to 160 KB of dynamic LDS: it opts in once per device
template <int K, int VEC, bool WAVE>
bool hg_opt_in() {
    static std::mutex mu;
    static int state[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return false; }
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
        state[dev] = 1;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_plane_histogram<K, VEC, WAVE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                HG_LDS_LIMIT) != hipSuccess) {
            (void)hipGetLastError();
            state[dev] = -1;
        }
    }
    return state[dev] == 1;
}

template <int K>
bool hg_launch(const HgArgs& a, bool vec, bool wave, size_t lds, hipStream_t st) {
    bool ok = true;
    rs::launch(a.rows, vec, wave, [&](dim3 grid, auto v, auto w) {
        ok = hg_opt_in<K, decltype(v)::value, decltype(w)::value>();
        if (ok) hipLaunchKernelGGL((k_plane_histogram<K, decltype(v)::value, decltype(w)::value>), grid, dim3(256), lds, st, a);
    });
    return ok;
}

}  // namespace

extern "C" int fg_plane_histogram(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz,
                                  int32_t ny, int32_t nx, const int32_t* rows, int32_t n_rows, const fg_real* lo, const fg_real* scale,
                                  int32_t bins, const int32_t* pairs, int32_t n_pairs, int32_t joint_bins, uint64_t* counts,
                                  uint64_t* joint, void* stream) {
    FG_REQUIRE(channels && batch_stride && rows, FG_ERR_INVALID_ARG, "fg_plane_histogram: null channel, stride or row table");
    FG_REQUIRE(lo && scale && counts, FG_ERR_INVALID_ARG, "fg_plane_histogram: null lo, scale or counts");
    FG_REQUIRE(n_pairs >= 0 && n_pairs <= HG_MAX_PAIRS, FG_ERR_INVALID_ARG, "fg_plane_histogram: n_pairs must be 0..6");
    FG_REQUIRE((joint != nullptr) == (n_pairs > 0), FG_ERR_INVALID_ARG, "fg_plane_histogram: joint must be given exactly when n_pairs > 0");
    FG_REQUIRE(n_pairs == 0 || pairs, FG_ERR_INVALID_ARG, "fg_plane_histogram: null pair table");
    FG_REQUIRE(K >= 1 && K <= HG_MAX_K, FG_ERR_INVALID_ARG, "fg_plane_histogram: K must be 1..5");
    FG_REQUIRE(bins >= 2 && bins <= HG_MAX_BINS, FG_ERR_INVALID_ARG, "fg_plane_histogram: bins must be 2..256");
    FG_REQUIRE(joint_bins >= 2 && joint_bins <= HG_MAX_JOINT_BINS && bins % joint_bins == 0, FG_ERR_INVALID_ARG,
               "fg_plane_histogram: joint_bins must be 2..64 and divide bins");
    FG_REQUIRE(batch > 0 && nz > 0 && ny > 0 && nx > 0, FG_ERR_INVALID_ARG, "fg_plane_histogram: batch, nz, ny, nx must be positive");
    FG_REQUIRE(n_rows >= 1 && n_rows <= ny, FG_ERR_INVALID_ARG, "fg_plane_histogram: n_rows must be 1..ny");
    for (int r = 0; r < n_rows; ++r) {
        FG_REQUIRE(rows[r] >= 0 && rows[r] < ny, FG_ERR_INVALID_ARG, "fg_plane_histogram: row index outside [0, ny)");
        FG_REQUIRE(r == 0 || rows[r] > rows[r - 1], FG_ERR_INVALID_ARG, "fg_plane_histogram: rows must be ascending and unique");
    }
    HgArgs a;
    for (int p = 0; p < HG_MAX_PAIRS; ++p) {
        a.pair[p][0] = a.pair[p][1] = 0;
        if (p >= n_pairs) continue;
        FG_REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < K && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < K, FG_ERR_INVALID_ARG,
                   "fg_plane_histogram: pair index outside [0, K)");
        a.pair[p][0] = (unsigned char)pairs[2 * p]; a.pair[p][1] = (unsigned char)pairs[2 * p + 1];
    }
    FG_REQUIRE((long long)nz * nx <= (1LL << 30), FG_ERR_INVALID_ARG, "fg_plane_histogram: a plane of more than 2^30 cells");
    FG_REQUIRE((long long)batch * n_rows <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_plane_histogram: batch * n_rows too large for one launch");
    bool vec;
    const int rc = rs::fill(a.t, vec, "fg_plane_histogram", "channel", channels, batch_stride, K, nz, ny, nx);
    if (rc != FG_OK) return rc;
    const bool wave = (long long)nz * nx <= rs::WAVE_CELLS;
    a.words = K * (bins + 3) + n_pairs * (joint_bins * joint_bins + 1);
    const size_t lds = (size_t)a.words * sizeof(unsigned) * (wave ? 4 : 1);
    FG_REQUIRE(lds <= (size_t)HG_LDS_LIMIT, FG_ERR_UNSUPPORTED,
               wave ? "fg_plane_histogram: 16 (K (bins + 3) + n_pairs (joint_bins^2 + 1)) bytes must fit in 160 KB of LDS (planes of up to 1024 cells)"
                    : "fg_plane_histogram: 4 (K (bins + 3) + n_pairs (joint_bins^2 + 1)) bytes must fit in 160 KB of LDS");
    a.zstride = (long long)ny * nx;
    a.nz = nz; a.nx = nx; a.n_rows = n_rows;
    a.bins = bins; a.n_pairs = n_pairs; a.joint_bins = joint_bins; a.jmul = 65536 / (bins / joint_bins) + 1;
    a.lo = lo; a.scale = scale; a.counts = (unsigned long long*)counts; a.joint = (unsigned long long*)joint;
    hipStream_t st = (hipStream_t)stream;
    for (int r0 = 0; r0 < n_rows; r0 += HG_ROW_CHUNK) {
        a.row0 = r0; a.ny = n_rows - r0 < HG_ROW_CHUNK ? n_rows - r0 : HG_ROW_CHUNK;
        a.rows = (long long)batch * a.ny;
        for (int q = 0; q < HG_ROW_CHUNK; ++q) a.row_of[q] = q < a.ny ? rows[r0 + q] : 0;
        bool ok;
        if (K == 1) ok = hg_launch<1>(a, vec, wave, lds, st);
        else if (K == 2) ok = hg_launch<2>(a, vec, wave, lds, st);
        else if (K == 3) ok = hg_launch<3>(a, vec, wave, lds, st);
        else if (K == 4) ok = hg_launch<4>(a, vec, wave, lds, st);
        else ok = hg_launch<5>(a, vec, wave, lds, st);
        FG_REQUIRE(ok, FG_ERR_HIP, "fg_plane_histogram: the device refused 160 KB of LDS per workgroup");
        FG_HIP_CHECK(hipGetLastError());
    }
    return FG_OK;
}
