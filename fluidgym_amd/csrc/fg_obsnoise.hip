// Counter-based Gaussian noise on the observations / actions of a batch (include/fluidgym_hip.h): dst = src + sigma z, where z
// is a pure function of (seed, row, that row's episode and step, tag of the tensor, element).  Nothing is remembered between launches
// but the per-row (episode, step) words the caller keeps on the device.
//
// The stream.  Element i of row r of segment s takes normal number i % 4 of the Philox4x32-10 block (Salmon et al., SC'11) with
//     key      (seed & 0xffffffff, seed >> 32)
//     counter  ((tag << 24) | (i / 4), row_id(r), counters[r][0], counters[r][1])
// tag < 256 and n <= 2^26 keep the first counter word free of collisions.
//
// The arithmetic of z, defined here once; tests/obs_noise_ref.py restates it operation for operation in np.float32.  Every fp32
// operation is rounded on its own (the file is compiled with -ffp-contract=off; hipcc's default float division and sqrtf are the
// correctly rounded ones); no logf / sinf / cosf of the math library, which are not reproducible off the device.  Words (w0, w1) of
// the block give (z0, z1), words (w2, w3) give (z2, z3):
//     u   = ((float)(w0 >> 9) + 0.5f) * 2^-23                                   exact, in (0, 1)
//     ln u: u = m 2^e by its bits, m in [1, 2);  if m > 1.41421354f: m = m * 0.5f, e = e + 1
//           t = (m - 1.0f) / (m + 1.0f);  t2 = t * t
//           p = (((L9 * t2 + L7) * t2 + L5) * t2 + L3) * t2 + 1.0f              L9, L7, L5, L3 = fp32(1/9, 1/7, 1/5, 1/3)
//           ln u = (float)e * 0.693147182f + (2.0f * t) * p
//     r   = sqrtf(-2.0f * ln u)
//     q   = w1 >> 30;  f = ((float)((w1 >> 9) & 0x1fffff) + 0.5f) * 2^-21        exact, in (0, 1): the angle is (q + f) pi / 2
//           swap = f > 0.5f;  if swap: f = 1.0f - f                              exact
//           a = f * 1.57079637f;  a2 = a * a
//           sn = ((((S9 * a2 + S7) * a2 + S5) * a2 + S3) * a2 + 1.0f) * a        S3, S5, S7, S9 = fp32(-1/6, 1/120, -1/5040, 1/362880)
//           cs = ((((C10 * a2 + C8) * a2 + C6) * a2 + C4) * a2 + C2) * a2 + 1.0f C2 .. C10 = fp32(-1/2, 1/24, -1/720, 1/40320, -1/3628800)
//           (c, s) = swap ? (sn, cs) : (cs, sn);  rotated by q: (c, s), (-s, c), (-c, -s), (s, -c)
//     z0  = r * c';  z1 = r * s'
// dtype 0: dst = src + (float)sigma * z in fp32;  dtype 1: dst = src + sigma * (double)z in fp64.  sigma == 0 runs the same arithmetic.
//
// Shape: observations are a few hundred to a few thousand elements per row, so the launch is bound by its latency and every tensor of a
// dict goes into ONE launch.  One lane per quad of four elements (one Philox block, four normals); the grid runs over (chunk of 256
// quads, row, segment), the segments sit in the kernel arguments and are read as wave-uniform scalars (a chunk past the end of a shorter
// segment returns at once).  A quad is loaded and stored as 16-byte words when base and strides allow it; otherwise, and for the tail
// quad, element by element.  No LDS, no atomics, nothing returns to the host.
#include "fg_internal.h"
#include "fg_philox.h"

namespace {

constexpr int NOISE_THREADS = 256;
constexpr int NOISE_MAX_SEG = 8;
constexpr int NOISE_MAX_N = 1 << 26;

struct NoiseSeg {
    const void* src;
    void* dst;
    long long src_stride, dst_stride;     // elements between rows
    int n;                                // elements per row
    uint32_t tag24;                       // tag << 24
    int vec;                              // both bases and both row pitches are multiples of 16 bytes
    double sigma;
};

struct NoiseArgs {
    NoiseSeg seg[NOISE_MAX_SEG];
    const uint32_t* counters;             // [rows][2] = (episode, step)
    const int32_t* row_ids;               // [rows] or null
    uint32_t key0, key1;
};

template <typename T>
__global__ __launch_bounds__(NOISE_THREADS) void k_obs_noise_add(const NoiseArgs a, int rows) {
    const NoiseSeg& sg = a.seg[blockIdx.z];                      // wave-uniform: segment, row, chunk
    const int row = blockIdx.y;
    const int quad = blockIdx.x * NOISE_THREADS + threadIdx.x;
    const long long i0 = 4LL * quad;
    if (row >= rows || i0 >= sg.n) return;
    const uint32_t rid = a.row_ids ? (uint32_t)a.row_ids[row] : (uint32_t)row;
    uint32_t w[4];
    philox4x32_10(sg.tag24 | (uint32_t)quad, rid, a.counters[2 * row], a.counters[2 * row + 1], a.key0, a.key1, w);
    float z[4];
    normal_pair(w[0], w[1], z[0], z[1]);
    normal_pair(w[2], w[3], z[2], z[3]);
    const T* src = static_cast<const T*>(sg.src) + (long long)row * sg.src_stride + i0;
    T* dst = static_cast<T*>(sg.dst) + (long long)row * sg.dst_stride + i0;
    if (sg.vec && i0 + 4 <= sg.n) {
        if constexpr (sizeof(T) == 4) {
            float4 v = *reinterpret_cast<const float4*>(src);
            v.x = add_noise(v.x, sg.sigma, z[0]); v.y = add_noise(v.y, sg.sigma, z[1]);
            v.z = add_noise(v.z, sg.sigma, z[2]); v.w = add_noise(v.w, sg.sigma, z[3]);
            *reinterpret_cast<float4*>(dst) = v;
        } else {
            double2 lo = reinterpret_cast<const double2*>(src)[0], hi = reinterpret_cast<const double2*>(src)[1];
            lo.x = add_noise(lo.x, sg.sigma, z[0]); lo.y = add_noise(lo.y, sg.sigma, z[1]);
            hi.x = add_noise(hi.x, sg.sigma, z[2]); hi.y = add_noise(hi.y, sg.sigma, z[3]);
            reinterpret_cast<double2*>(dst)[0] = lo;
            reinterpret_cast<double2*>(dst)[1] = hi;
        }
    } else {
        const int left = (int)(sg.n - i0 < 4 ? sg.n - i0 : 4);
        T v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) v[j] = src[j];                         // every load of the quad before its first store (dst may be src)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) dst[j] = add_noise(v[j], sg.sigma, z[j]);
    }
}

}  // namespace

extern "C" int fg_obs_noise_add(const fg_noise_segment* seg, int32_t n_seg, int32_t rows, int32_t dtype, uint64_t seed,
                                const uint32_t* counters, const int32_t* row_ids, void* stream) {
    FG_REQUIRE(seg && counters, FG_ERR_INVALID_ARG, "fg_obs_noise_add: null argument (seg and counters are required)");
    FG_REQUIRE(n_seg >= 1 && n_seg <= NOISE_MAX_SEG, FG_ERR_INVALID_ARG,
               "fg_obs_noise_add: n_seg = " + std::to_string(n_seg) + " is outside [1, " + std::to_string(NOISE_MAX_SEG) + "]");
    FG_REQUIRE(rows >= 1 && rows <= 65535, FG_ERR_INVALID_ARG, "fg_obs_noise_add: rows = " + std::to_string(rows) + " is outside [1, 65535]");
    FG_REQUIRE(dtype == 0 || dtype == 1, FG_ERR_INVALID_ARG, "fg_obs_noise_add: dtype must be 0 (float) or 1 (double)");
    const size_t elem = dtype == 0 ? 4 : 8;
    NoiseArgs a{};
    int max_n = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
        const fg_noise_segment& g = seg[s];
        const std::string who = "fg_obs_noise_add: segment " + std::to_string(s);
        FG_REQUIRE(g.src && g.dst, FG_ERR_INVALID_ARG, who + ": null src or dst");
        FG_REQUIRE(g.n >= 1 && g.n <= NOISE_MAX_N, FG_ERR_INVALID_ARG, who + ": n = " + std::to_string(g.n) + " is outside [1, 2^26]");
        FG_REQUIRE(g.tag < 256, FG_ERR_INVALID_ARG, who + ": tag = " + std::to_string(g.tag) + " must be below 256");
        FG_REQUIRE(g.src_stride >= g.n && g.dst_stride >= g.n, FG_ERR_INVALID_ARG,
                   who + ": a stride (" + std::to_string(g.src_stride) + ", " + std::to_string(g.dst_stride) + ") is smaller than n = " +
                       std::to_string(g.n));
        NoiseSeg& k = a.seg[s];
        k.src = g.src; k.dst = g.dst; k.src_stride = g.src_stride; k.dst_stride = g.dst_stride;
        k.n = g.n; k.tag24 = g.tag << 24; k.sigma = g.sigma;
        k.vec = (reinterpret_cast<uintptr_t>(g.src) % 16 == 0 && reinterpret_cast<uintptr_t>(g.dst) % 16 == 0 &&
                 ((size_t)g.src_stride * elem) % 16 == 0 && ((size_t)g.dst_stride * elem) % 16 == 0) ? 1 : 0;
        max_n = g.n > max_n ? g.n : max_n;
    }
    a.counters = counters; a.row_ids = row_ids;
    a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32);
    const unsigned quads = (unsigned)((max_n + 3) / 4);
    const dim3 grid((quads + NOISE_THREADS - 1) / NOISE_THREADS, (unsigned)rows, (unsigned)n_seg);
    if (dtype == 0) hipLaunchKernelGGL(k_obs_noise_add<float>, grid, dim3(NOISE_THREADS), 0, (hipStream_t)stream, a, (int)rows);
    else hipLaunchKernelGGL(k_obs_noise_add<double>, grid, dim3(NOISE_THREADS), 0, (hipStream_t)stream, a, (int)rows);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
