// The two classical baseline controllers of the benchmarks (fluidgym_amd/baselines.py), one launch per action for
// the whole batch, nothing returned to the host:
//
//   fg_baseline_opposition   opposition control of the turbulent channel: action[b, w, i, j] = gain[w] (P[i, j] - m) with m the mean of
//                            the wall-normal velocity over the detection plane (z, x) at row rows[w] and P[i, j] its mean over the
//                            actuator patch x in [i actor, (i + 1) actor), z in [j actor, (j + 1) actor)
//   fg_baseline_pd           PD control of Rayleigh-Benard convection: E[b, hz, hx] = sum_y wy[y] mean_{z, x over the heater} v, the
//                            height-averaged vertical velocity above heater (hz, hx); action = -(kp E + kd/dt (E - E_previous))
//
// Order: fp64 sums in a fixed tree (fg_rowstat.h: every lane its cells in ascending order, the xor butterfly of the wave, the four waves
// in ascending order), no floating-point atomic, one rounding to fg_real at the end.  What a thread sums is decided by the extents alone;
// the load form (one 16-byte load or single reals, by the alignment) changes no operation, so both forms give the same bits (this file
// is compiled with -ffp-contract=off: every product and sum rounded on its own, in every template instance).
//
// Opposition control: one workgroup per (env, wall).  A thread owns strips of the plane, `az` rows of z by `width` cells of x holding G
// whole patches: G = VEC / actor where actor < VEC divides VEC and VEC divides nx (a 16-byte load then spans G patches), else G = 1 and
// the strip is the patch.  A patch sum adds its cells with z ascending, then x ascending; the plane sum is the sum of the patch sums
// (a thread's patches in ascending order, then the tree).  The patch sums are taken a second time, in the same order, for the output:
// the plane is a few hundred KB at most and sits in L2.
//
// PD control: one wave (columns of up to WAVE_CELLS cells) or one workgroup per (env, heater).  first[env] is read by every heater of the
// env; the heater that draws the last ticket of the call clears it (the rule of FG_ROWSTAT_ADVANCE_N).
#include "fg_rowstat.h"

namespace {

namespace rs = fg_rowstat;

// C consecutive reals at p as doubles: V == C one 16-byte load, V == 1 single loads
template <int V, int C>
__device__ __forceinline__ void bl_cells(const fg_real* p, double (&c)[C]) {
    if constexpr (V == C) {
        rs::load<C>(p, c);
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = (double)p[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- opposition control
struct OcArgs {
    const fg_real* v;
    long long bstride, zstride;          // batch stride; ny * nx
    int nz, nx, actor, az, n_walls, nax, naz;
    int row0, row1;
    double gain0, gain1;
    fg_real* action;
};

// the sums S[g] of the G patches of strip s (nsx strips per z block of the plane)
template <int V, int G>
__device__ __forceinline__ void oc_strip(const OcArgs& a, const fg_real* plane, int s, int nsx, int& sz, int& sx, double (&S)[G]) {
    constexpr int A = rs::VEC / G;                           // G > 1: the patch edge along x
    const int width = G > 1 ? rs::VEC : a.actor;
    sz = s / nsx; sx = s - sz * nsx;
    const fg_real* p = plane + (long long)sz * a.az * a.zstride + (long long)sx * width;
#pragma unroll
    for (int g = 0; g < G; ++g) S[g] = 0.0;
    for (int dz = 0; dz < a.az; ++dz, p += a.zstride) {
        if constexpr (G > 1) {
            double c[rs::VEC];
            bl_cells<V, rs::VEC>(p, c);
#pragma unroll
            for (int k = 0; k < rs::VEC; ++k) S[k / A] += c[k];
        } else if constexpr (V > 1) {
            for (int x = 0; x < a.actor; x += V) {
                double c[V];
                rs::load<V>(p + x, c);
#pragma unroll
                for (int k = 0; k < V; ++k) S[0] += c[k];
            }
        } else {
            for (int x = 0; x < a.actor; ++x) S[0] += (double)p[x];
        }
    }
}

template <int V, int G>
__global__ __launch_bounds__(256) void k_baseline_opposition(OcArgs a) {
    __shared__ double s_red[4][1];
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x / a.n_walls, w = (int)blockIdx.x - b * a.n_walls;
    const fg_real* plane = a.v + (long long)b * a.bstride + (long long)(w ? a.row1 : a.row0) * a.nx;
    const int nsx = a.nx / (G > 1 ? rs::VEC : a.actor), strips = a.naz * nsx;
    int sz, sx;
    double S[G], total[1] = {0.0};
    for (int s = tid; s < strips; s += 256) {
        oc_strip<V, G>(a, plane, s, nsx, sz, sx, S);
#pragma unroll
        for (int g = 0; g < G; ++g) total[0] += S[g];
    }
    rs::reduce<1, 1, false>(total, s_red, tid);
    const double m = total[0] / ((double)a.nz * (double)a.nx), cells = (double)a.az * (double)a.actor, gain = w ? a.gain1 : a.gain0;
    fg_real* out = a.action + (long long)blockIdx.x * a.nax * a.naz;
    for (int s = tid; s < strips; s += 256) {
        oc_strip<V, G>(a, plane, s, nsx, sz, sx, S);
#pragma unroll
        for (int g = 0; g < G; ++g) out[(long long)(sx * G + g) * a.naz + sz] = (fg_real)(gain * (S[g] / cells - m));
    }
}

template <int V>
void oc_launch(const OcArgs& a, int G, dim3 grid, hipStream_t st) {
    if (G == 1) hipLaunchKernelGGL((k_baseline_opposition<V, 1>), grid, dim3(256), 0, st, a);
    else if (G == 2) hipLaunchKernelGGL((k_baseline_opposition<V, 2>), grid, dim3(256), 0, st, a);
    else if constexpr (rs::VEC == 4) hipLaunchKernelGGL((k_baseline_opposition<V, 4>), grid, dim3(256), 0, st, a);
}

// ------------------------------------------------------------------------------------------------------------------------ PD control
struct PdArgs {
    const fg_real* v;
    long long bstride, zstride, rows;    // batch stride; ny * nx; batch * nhz * nhx
    int ny, nx, seg, segz, nhz, nhx;
    const double* wy;
    double kp, kd_over_dt;
    double* e_state;
    int32_t* first;
    unsigned long long* tickets;
    fg_real* action;
};

// C: the cells of a work item (VEC where VEC divides seg, by the extents alone); V: those of a load
template <int V, int C, bool WAVE>
__global__ __launch_bounds__(256) void k_baseline_pd(PdArgs a) {
    __shared__ double s_red[4][1];
    const int tid = threadIdx.x;
    const long long h = WAVE ? (long long)blockIdx.x * 4 + (tid >> 6) : (long long)blockIdx.x;
    if (WAVE && h >= a.rows) return;                        // a wave without a heater leaves as a whole; that form has no barrier
    const int per_env = a.nhz * a.nhx;
    const int b = (int)(h / per_env), hh = (int)(h - (long long)b * per_env), hz = hh / a.nhx, hx = hh - hz * a.nhx;
    const fg_real* col = a.v + (long long)b * a.bstride + (long long)hz * a.segz * a.zstride + (long long)hx * a.seg;
    const int nxc = a.seg / C, items = a.segz * a.ny * nxc;
    const int t0 = WAVE ? (tid & 63) : tid, step = WAVE ? 64 : 256;
    double e[1] = {0.0};
    for (int i = t0; i < items; i += step) {
        const int line = i / nxc, xc = i - line * nxc, z = line / a.ny, y = line - z * a.ny;
        const double w = a.wy[y];
        double c[C];
        bl_cells<V, C>(col + (long long)z * a.zstride + (long long)y * a.nx + xc * C, c);
#pragma unroll
        for (int k = 0; k < C; ++k) e[0] += w * c[k];
    }
    rs::reduce<1, 1, WAVE>(e, s_red, tid);
    if (t0 != 0) return;
    const double E = e[0] / ((double)a.seg * (double)a.segz);
    const double d = a.first[b] ? 0.0 : a.kd_over_dt * (E - a.e_state[h]);
    a.action[h] = (fg_real)(-(a.kp * E + d));
    a.e_state[h] = E;
    // every heater of env b has read first[b] before it takes its ticket; the one that draws the last ticket of this call clears it
    const unsigned long long ticket = __hip_atomic_fetch_add(&a.tickets[b], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if ((ticket + 1ull) % (unsigned long long)per_env == 0ull) a.first[b] = 0;
}

template <int V, int C>
void pd_launch(const PdArgs& a, bool wave, hipStream_t st) {
    if (wave) hipLaunchKernelGGL((k_baseline_pd<V, C, true>), dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_baseline_pd<V, C, false>), dim3((unsigned)a.rows), dim3(256), 0, st, a);
}

// the checks both entry points share; edge: actor / seg
int bl_check_grid(const char* entry, const fg_real* v, int64_t batch_stride, int batch, int nz, int ny, int nx, int edge, const char* edge_name) {
    const std::string e(entry);
    FG_REQUIRE(v, FG_ERR_INVALID_ARG, e + ": null field pointer");
    FG_REQUIRE(batch >= 1 && nz > 0 && ny > 0 && nx > 0, FG_ERR_INVALID_ARG, e + ": batch, nz, ny, nx must be positive");
    FG_REQUIRE(edge >= 1, FG_ERR_INVALID_ARG, e + ": " + edge_name + " must be at least 1");
    FG_REQUIRE(nx % edge == 0 && (nz == 1 || nz % edge == 0), FG_ERR_INVALID_ARG, e + ": " + edge_name + " must divide nx (and nz where nz > 1)");
    FG_REQUIRE((long long)nz * nx <= (1LL << 30), FG_ERR_INVALID_ARG, e + ": a plane of more than 2^30 cells");
    FG_REQUIRE(batch_stride >= (long long)nz * ny * nx, FG_ERR_INVALID_ARG, e + ": batch stride smaller than nz * ny * nx");
    return FG_OK;
}

}  // namespace

extern "C" int fg_baseline_opposition(const fg_real* v, int64_t batch_stride, int32_t batch, int32_t nz, int32_t ny, int32_t nx,
                                      const int32_t* rows, const double* gain, int32_t n_walls, int32_t actor, fg_real* action,
                                      void* stream) {
    FG_REQUIRE(rows && gain && action, FG_ERR_INVALID_ARG, "fg_baseline_opposition: null rows, gain or action pointer");
    FG_REQUIRE(n_walls == 1 || n_walls == 2, FG_ERR_INVALID_ARG, "fg_baseline_opposition: n_walls must be 1 or 2");
    const int rc = bl_check_grid("fg_baseline_opposition", v, batch_stride, batch, nz, ny, nx, actor, "actor");
    if (rc != FG_OK) return rc;
    for (int w = 0; w < n_walls; ++w)
        FG_REQUIRE(rows[w] >= 0 && rows[w] < ny, FG_ERR_INVALID_ARG, "fg_baseline_opposition: a detection row outside [0, ny)");
    FG_REQUIRE((long long)batch * n_walls <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_baseline_opposition: batch * n_walls too large for one launch");
    OcArgs a;
    a.v = v; a.bstride = (long long)batch_stride; a.zstride = (long long)ny * nx;
    a.nz = nz; a.nx = nx; a.actor = actor; a.az = nz > 1 ? actor : 1; a.n_walls = n_walls;
    a.nax = nx / actor; a.naz = nz / a.az;
    a.row0 = rows[0]; a.row1 = rows[n_walls - 1];
    a.gain0 = gain[0]; a.gain1 = gain[n_walls - 1];
    a.action = action;
    const int G = (actor < rs::VEC && rs::VEC % actor == 0 && nx % rs::VEC == 0) ? rs::VEC / actor : 1;      // by the extents alone
    const bool vec = nx % rs::VEC == 0 && (G > 1 || actor % rs::VEC == 0) && (uintptr_t)v % 16 == 0 && batch_stride % rs::VEC == 0;
    const dim3 grid((unsigned)(batch * n_walls));
    hipStream_t st = (hipStream_t)stream;
    if (vec) oc_launch<rs::VEC>(a, G, grid, st);
    else oc_launch<1>(a, G, grid, st);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_baseline_pd(const fg_real* v, int64_t batch_stride, int32_t batch, int32_t nz, int32_t ny, int32_t nx, int32_t seg,
                              const double* wy, double kp, double kd_over_dt, double* e_state, int32_t* first, uint64_t* tickets,
                              fg_real* action, void* stream) {
    FG_REQUIRE(wy && e_state && first && tickets && action, FG_ERR_INVALID_ARG,
               "fg_baseline_pd: null wy, e_state, first, tickets or action pointer");
    const int rc = bl_check_grid("fg_baseline_pd", v, batch_stride, batch, nz, ny, nx, seg, "seg");
    if (rc != FG_OK) return rc;
    PdArgs a;
    a.v = v; a.bstride = (long long)batch_stride; a.zstride = (long long)ny * nx;
    a.ny = ny; a.nx = nx; a.seg = seg; a.segz = nz > 1 ? seg : 1; a.nhz = nz / a.segz; a.nhx = nx / seg;
    a.rows = (long long)batch * a.nhz * a.nhx;
    FG_REQUIRE(a.rows <= 0x7fffffffLL, FG_ERR_INVALID_ARG, "fg_baseline_pd: batch * heaters too large for one launch");
    FG_REQUIRE((long long)a.segz * ny * seg <= (1LL << 30), FG_ERR_INVALID_ARG, "fg_baseline_pd: a heater column of more than 2^30 cells");
    a.wy = wy; a.kp = kp; a.kd_over_dt = kd_over_dt;
    a.e_state = e_state; a.first = first; a.tickets = (unsigned long long*)tickets; a.action = action;
    const bool wide = seg % rs::VEC == 0;                                                                    // by the extents alone
    const bool vec = wide && nx % rs::VEC == 0 && (uintptr_t)v % 16 == 0 && batch_stride % rs::VEC == 0;
    const bool wave = (long long)a.segz * ny * seg <= rs::WAVE_CELLS;
    hipStream_t st = (hipStream_t)stream;
    if (vec) pd_launch<rs::VEC, rs::VEC>(a, wave, st);
    else if (wide) pd_launch<1, rs::VEC>(a, wave, st);
    else pd_launch<1, 1>(a, wave, st);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
