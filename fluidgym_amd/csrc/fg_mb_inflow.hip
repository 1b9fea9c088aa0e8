// Per-env unsteady inflow of a multi-block handle (include/fluidgym_hip.h): the prescribed values of one FIXED face --
// the inflow of the cylinder and airfoil envs -- become a steady base profile times a gust, env by env, and the outflow faces are
// rescaled so that the boundary fluxes of every env sum to zero again, which is what the guard at the top of fg_mb_single_step asks
// before the step's own PRE hook runs.  ONE launch per sim step for the whole batch, one workgroup of FG_BLOCK threads per env,
// four phases separated by barriers.
//
// 1. Signals.  Env b has K_s streamwise modes (a, f, phi) and K_t transverse modes (g, h, psi), K <= 8, read from a device table
//    [B][6][8] of doubles (rows a, f, phi, g, h, psi) or drawn (below).  Lane k < 8 prepares mode k of both families.  The time is
//    t = n dt in double with n = counters[b][0] * sim_steps + k_sim (64-bit), the sim steps env b has taken in its episode.
//        S    = sum_k a_k sin2pi(frac(f_k t + phi_k))                        k = 0 .. K_s-1, summed in that order from 0.0f
//        G(y) = sum_k g_k sin2pi(frac((h_k t + psi_k) - kappa y))            k = 0 .. K_t-1, likewise
//    The argument is formed in double, every operation rounded on its own (the file is compiled with -ffp-contract=off),
//    frac(x) = x - floor(x), then cast to float: p in [0, 1].  sin2pi(p) in fp32: p4 = p * 4.0f, q = (int)p4, fr = p4 - (float)q (both
//    exact), q = q & 3; the angle is (q + fr) pi / 2, folded and evaluated by the quarter-wave rule and the polynomials of
//    fg_obsnoise.hip: swap = fr > 0.5f; if swap: fr = 1.0f - fr; a = fr * 1.57079637f; sn, cs as there; s = swap ? cs : sn,
//    c = swap ? sn : cs; the sine is s, c, -s, -c for q = 0, 1, 2, 3.  Amplitudes are floats; a term is a_k * sine, one product.
//    Signals are fp32 in both libraries.
// 2. Inflow slots sl = slot0 + s, s in [0, count), with base in the layout of the boundary velocity and y[s] the face centre:
//        ub[b][0][sl] = base[b][0][sl] * (mb_real)(1.0f + S)
//        ub[b][1][sl] = base[b][1][sl] + base[b][0][sl] * (mb_real)G(y[s])
//        ub[b][c][sl] = base[b][c][sl]                                        c >= 2
// 3. The signed boundary fluxes of env b over all NB slots, split into fixed and free (the up to two outflow ranges): the loop and
//    the block sum of k_mb_bflux (fg_mb_step.hip), so the order of the sums is fixed.
// 4. If |fixed + free| > atol = 0.01f * outflow_tol (what mb_outflow_pre hands k_mb_balance), every component of the outflow slots is
//    multiplied by -fixed / free: the rule of k_mb_balance.  The advective update of the outflow (k_mb_outflow) is NOT run here: it
//    stays with the step's PRE hook.
// signal[b] = (S, G(y_mid)) is written by lane 0.  No atomics, nothing returns to the host.
//
// The random form (modes == NULL).  The modes of env b are a pure function of (seed, r = env_offset + b, e = counters[b][1]): mode k
// takes the Philox4x32-10 block with key (seed low, seed high) and counter ((FG_INFLOW_TAG << 24) | k, r, e, 0), FG_INFLOW_TAG = 240
// (the observation keys use tags below 128, the action 128, the reset noise 0 .. 3 with a last word of 0xFFFFFFFF).  Word j becomes
// u_j = ((float)(w_j >> 9) + 0.5f) * 2^-23, exact, in (0, 1), and in double
//     f_k = f_lo + (((double)k + u_0) * (f_hi - f_lo)) / (double)K_s        phi_k = u_1
//     h_k = f_lo + (((double)k + u_2) * (f_hi - f_lo)) / (double)K_t        psi_k = u_3
// with a_k = (float)(streamwise_rms * sqrt(2.0 / K_s)) and g_k = (float)(transverse_rms * sqrt(2.0 / K_t)) formed once on the host.
#include <cmath>

#include "fg_mb_solve.h"
#include "fg_philox.h"

namespace {

constexpr int MI_MAX_MODES = 8;
constexpr uint32_t MI_TAG = 240;

struct MiArgs {
    int slot0, count;
    int out0, outn, out0b, outnb;
    int ks, kt;
    int sim_steps, k_sim;
    uint32_t env_offset, key0, key1;
    float amp_s, amp_t;                   // random form: a_k, g_k
    double dt, f_lo, f_hi, kappa, y_mid;
    mb_real atol;
    const mb_real* base;
    const double* y;
    const double* modes;
    const uint32_t* counters;
    float* signal;
};

// sin(2 pi frac(x)): the definition at the top of this file, in its order
__device__ __forceinline__ float sin2pi_frac(double x) {
    const double fr64 = x - floor(x);
    const float p = (float)fr64;
    const float p4 = p * 4.0f;
    int q = (int)p4;
    float f = p4 - (float)q;
    q &= 3;
    const bool swap = f > 0.5f;
    if (swap) f = 1.0f - f;
    const float a = f * 1.57079637f;
    const float a2 = a * a;
    float sn = (float)(1.0 / 362880.0) * a2 + (float)(-1.0 / 5040.0);
    sn = sn * a2 + (float)(1.0 / 120.0);
    sn = sn * a2 + (float)(-1.0 / 6.0);
    sn = sn * a2 + 1.0f;
    sn = sn * a;
    float cs = (float)(-1.0 / 3628800.0) * a2 + (float)(1.0 / 40320.0);
    cs = cs * a2 + (float)(-1.0 / 720.0);
    cs = cs * a2 + (float)(1.0 / 24.0);
    cs = cs * a2 + -0.5f;
    cs = cs * a2 + 1.0f;
    const float s = swap ? cs : sn, c = swap ? sn : cs;
    return (q == 0) ? s : (q == 1) ? c : (q == 2) ? -s : -c;
}

template <int DIMS>
__global__ __launch_bounds__(FG_BLOCK) void k_mb_inflow(MbDev D, const MiArgs a, mb_real* ub) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float s_term[MI_MAX_MODES], s_g[MI_MAX_MODES];
    __shared__ double s_arg[MI_MAX_MODES];
    __shared__ mb_real lds[4];
    // ---- 1. signals: lane k prepares mode k of both families
    if (tid < MI_MAX_MODES) {
        const unsigned long long n = (unsigned long long)a.counters[2 * b] * (unsigned long long)a.sim_steps + (unsigned long long)a.k_sim;
        const double t = (double)n * a.dt;
        double f, phi, h, psi;
        float ak, gk;
        if (a.modes) {
            const double* m = a.modes + (size_t)b * 6 * MI_MAX_MODES + tid;
            ak = (float)m[0]; f = m[MI_MAX_MODES]; phi = m[2 * MI_MAX_MODES];
            gk = (float)m[3 * MI_MAX_MODES]; h = m[4 * MI_MAX_MODES]; psi = m[5 * MI_MAX_MODES];
        } else {
            uint32_t w[4];
            philox4x32_10((MI_TAG << 24) | (uint32_t)tid, a.env_offset + (uint32_t)b, a.counters[2 * b + 1], 0u, a.key0, a.key1, w);
            double u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = (double)(((float)(w[j] >> 9) + 0.5f) * 0x1p-23f);
            const double width = a.f_hi - a.f_lo;
            f = a.f_lo + (((double)tid + u[0]) * width) / (double)a.ks;
            phi = u[1];
            h = a.f_lo + (((double)tid + u[2]) * width) / (double)a.kt;
            psi = u[3];
            ak = a.amp_s; gk = a.amp_t;
        }
        s_term[tid] = tid < a.ks ? ak * sin2pi_frac(f * t + phi) : 0.0f;
        s_g[tid] = tid < a.kt ? gk : 0.0f;
        s_arg[tid] = tid < a.kt ? h * t + psi : 0.0;
    }
    __syncthreads();
    float S = 0.0f;
    for (int k = 0; k < a.ks; ++k) S += s_term[k];
    auto gust = [&](double y) {
        float G = 0.0f;
        for (int k = 0; k < a.kt; ++k) G += s_g[k] * sin2pi_frac(s_arg[k] - a.kappa * y);
        return G;
    };
    if (tid == 0) { a.signal[2 * b] = S; a.signal[2 * b + 1] = gust(a.y_mid); }
    // ---- 2. the inflow slots
    const mb_real gain = (mb_real)(1.0f + S);
    for (int s = tid; s < a.count; s += FG_BLOCK) {
        const int sl = a.slot0 + s;
        const mb_real b0 = a.base[((size_t)b * DIMS + 0) * D.NB + sl];
        const mb_real G = (mb_real)gust(a.y[s]);
        ub[((size_t)b * DIMS + 0) * D.NB + sl] = b0 * gain;
        ub[((size_t)b * DIMS + 1) * D.NB + sl] = a.base[((size_t)b * DIMS + 1) * D.NB + sl] + b0 * G;
#pragma unroll
        for (int c = 2; c < DIMS; ++c) ub[((size_t)b * DIMS + c) * D.NB + sl] = a.base[((size_t)b * DIMS + c) * D.NB + sl];
    }
    __syncthreads();
    // ---- 3. boundary fluxes (k_mb_bflux)
    mb_real fx = 0.f, fr = 0.f;
    for (int sl = tid; sl < D.NB; sl += FG_BLOCK) {
        const mb_real* t = D.Tb + (size_t)sl * (DIMS * DIMS + 1);
        const int f = D.bface[sl], axis = f >> 1;
        mb_real s = 0.f;
#pragma unroll
        for (int c = 0; c < DIMS; ++c) s += t[axis * DIMS + c] * ub[((size_t)b * DIMS + c) * D.NB + sl];
        s *= t[DIMS * DIMS] * ((f & 1) ? 1.f : -1.f);
        if ((sl >= a.out0 && sl < a.out0 + a.outn) || (sl >= a.out0b && sl < a.out0b + a.outnb)) fr += s; else fx += s;
    }
    fx = mb_block_sum(fx, lds);
    fr = mb_block_sum(fr, lds);
    // ---- 4. rebalance the outflow (k_mb_balance)
    if (mb_fabs(fx + fr) <= a.atol) return;
    const mb_real scale = -fx / fr;
    const int r0[2] = {a.out0, a.out0b}, rn[2] = {a.outn, a.outnb};
#pragma unroll
    for (int r = 0; r < 2; ++r)
        for (int k = tid; k < rn[r]; k += FG_BLOCK) {
#pragma unroll
            for (int c = 0; c < DIMS; ++c) ub[((size_t)b * DIMS + c) * D.NB + r0[r] + k] *= scale;
        }
}

bool ranges_overlap(int a0, int an, int b0, int bn) { return an > 0 && bn > 0 && a0 < b0 + bn && b0 < a0 + an; }

}  // namespace

extern "C" int fg_mb_inflow_disturbance(fg_mb_handle s, const fg_mb_inflow_params* p, void* stream) {
    const std::string who = "fg_mb_inflow_disturbance: ";
    FG_REQUIRE(s != nullptr, FG_ERR_INVALID_ARG, who + "null handle");
    FG_REQUIRE(p != nullptr, FG_ERR_INVALID_ARG, who + "null parameters");
    FG_REQUIRE(p->n_streamwise >= 0 && p->n_streamwise <= MI_MAX_MODES && p->n_transverse >= 0 && p->n_transverse <= MI_MAX_MODES,
               FG_ERR_INVALID_ARG, who + "n_streamwise = " + std::to_string(p->n_streamwise) + ", n_transverse = " +
                                       std::to_string(p->n_transverse) + ": the mode counts must be in 0..8");
    FG_REQUIRE(p->count > 0, FG_ERR_INVALID_ARG, who + "count = " + std::to_string(p->count) + ": the inflow face has no slots");
    FG_REQUIRE(std::isfinite(p->dt) && p->dt >= 0.0, FG_ERR_INVALID_ARG, who + "dt is negative or not finite");
    FG_REQUIRE(p->sim_steps >= 1 && p->k >= 0 && p->k < p->sim_steps, FG_ERR_INVALID_ARG, who + "sim_steps must be positive and k in [0, sim_steps)");
    FG_REQUIRE(std::isfinite(p->kappa) && std::isfinite(p->y_mid) && std::isfinite(p->outflow_tol) && p->outflow_tol >= 0.0,
               FG_ERR_INVALID_ARG, who + "kappa, y_mid or outflow_tol is not finite");
    if (!p->modes && (p->n_streamwise > 0 || p->n_transverse > 0))
        FG_REQUIRE(std::isfinite(p->f_lo) && std::isfinite(p->f_hi) && p->f_lo >= 0.0 && p->f_hi >= p->f_lo &&
                       std::isfinite(p->streamwise_rms) && p->streamwise_rms >= 0.0 && std::isfinite(p->transverse_rms) && p->transverse_rms >= 0.0,
                   FG_ERR_INVALID_ARG, who + "the band must be finite with 0 <= f_lo <= f_hi, the rms amplitudes finite and non-negative");
    FG_REQUIRE(p->base && p->y && p->counters && p->signal, FG_ERR_INVALID_ARG, who + "null base, y, counters or signal");
    FG_REQUIRE(s->finalized, FG_ERR_NOT_BOUND, who + "the handle is not finalised");
    FG_REQUIRE(p->slot0 >= 0 && p->slot0 + p->count <= s->NB, FG_ERR_INVALID_ARG, who + "inflow slots out of range");
    FG_REQUIRE(p->outflow_slot0 >= 0 && p->outflow_count > 0 && p->outflow_slot0 + p->outflow_count <= s->NB && p->outflow_count_b >= 0 &&
                   (p->outflow_count_b == 0 || (p->outflow_slot0_b >= 0 && p->outflow_slot0_b + p->outflow_count_b <= s->NB)),
               FG_ERR_INVALID_ARG, who + "outflow slots out of range");
    FG_REQUIRE(!ranges_overlap(p->slot0, p->count, p->outflow_slot0, p->outflow_count) &&
                   !ranges_overlap(p->slot0, p->count, p->outflow_slot0_b, p->outflow_count_b) &&
                   !ranges_overlap(p->outflow_slot0, p->outflow_count, p->outflow_slot0_b, p->outflow_count_b),
               FG_ERR_INVALID_ARG, who + "the inflow and outflow slot ranges overlap");
    FG_REQUIRE(!s->host_only && s->bvel, FG_ERR_NOT_BOUND, who + "the fields are not bound (fg_mb_bind)");
    MiArgs a{};
    a.slot0 = p->slot0; a.count = p->count;
    a.out0 = p->outflow_slot0; a.outn = p->outflow_count; a.out0b = p->outflow_slot0_b; a.outnb = p->outflow_count_b;
    a.ks = p->n_streamwise; a.kt = p->n_transverse;
    a.sim_steps = p->sim_steps; a.k_sim = p->k;
    a.env_offset = (uint32_t)p->env_offset;
    a.key0 = (uint32_t)(p->seed & 0xffffffffu); a.key1 = (uint32_t)(p->seed >> 32);
    a.amp_s = a.ks > 0 ? (float)(p->streamwise_rms * std::sqrt(2.0 / (double)a.ks)) : 0.0f;
    a.amp_t = a.kt > 0 ? (float)(p->transverse_rms * std::sqrt(2.0 / (double)a.kt)) : 0.0f;
    a.dt = p->dt; a.f_lo = p->f_lo; a.f_hi = p->f_hi; a.kappa = p->kappa; a.y_mid = p->y_mid;
    a.atol = 0.01f * (mb_real)p->outflow_tol;
    a.base = (const mb_real*)p->base; a.y = p->y; a.modes = p->modes; a.counters = p->counters; a.signal = p->signal;
    hipStream_t st = (hipStream_t)stream;
    MB_DISPATCH(s, hipLaunchKernelGGL(k_mb_inflow<DIMS>, dim3(s->B), dim3(FG_BLOCK), 0, st, s->dev, a, s->bvel););
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
