// Point probes and Lagrangian tracers on a curvilinear multi-block mesh (fluidgym_amd/simulation/mb_tracers.py),
// handle-free, both libraries:
//
//   fg_mb_point_locate    position -> (cell, xi, status): a walk over the mesh's neighbour table from a start cell
//   fg_mb_point_sample    out[b, p, :] = (u, v(, w), extra fields) at located points (cell, xi): the gather alone
//   fg_mb_tracer_advect   `substeps` midpoint steps of every tracer in the frozen velocity field, each position located by a walk
//
// The interpolant.  A field has a value at every mesh vertex v, sum_k w_vk phi_k over a stencil the host built (ELL tables, weights
// of zero are padding and are skipped): the cells that touch v, or -- for the velocity at a vertex on a FIXED face -- the boundary
// slots that touch v and nothing else (an index >= N names slot index - N).  The value at a point of a cell is the multilinear blend of
// the cell's 2^d vertex values with the local coordinates xi, x first, then y, then z, a + w (b - a) and b itself at w == 1.
//
// The walk.  In a cell, Newton on the cell's own bi- / trilinear map from xi = 1/2: at most 8 iterations, every iterate clamped to
// [-1, 2]^d, stopped once the step is below slack / 4.  xi in [-slack, 1 + slack]^d: found.  Else the faces violated by more than
// slack are tried in the order of their violation (the lower face index first among equals): a face with a neighbour is taken -- the
// position is shifted by the face's periodic vector where it has one, and the crossing counted --, a FIXED face is passed over; if
// every violated face is FIXED the point is outside and stays in this cell (status 1, the slot of the most violated face).  A walk
// that steps back into the cell it has just left accepts that cell after its Newton run.  More than max_walk cell changes, or a xi
// that is a NaN: status 2.  On return xi is clamped to [0, 1]^d (a NaN becomes 0).
//
// A position becomes an index in no other way: cell indices handed in are clamped to 0 .. N - 1 before any load, every other index
// comes from a table of the host, a NaN compares false with every bound and ends the walk where it stands.
//
// Shape: one thread per point / tracer, grid (ceil(n / 256), batch); blockIdx.y is the env, so the mesh record (a kernel argument:
// scalar registers) and every base pointer are wave-uniform.  The mesh tables are read-only, shared by the batch, and sit in L2; the
// walk diverges per lane and keeps the state of its cell in registers (every array below is indexed by unrolled loops only): no LDS.
// No floating-point atomic: the only atomic is the integer count of lost tracers.  Nothing returns to the host.  Every product and
// sum is rounded on its own (-ffp-contract=off in the Makefile): the NumPy restatement of the tests follows the same operations.
#include "fg_internal.h"

namespace {

constexpr int MBT_BLOCK = 256, MBT_MAX_EXTRA = 8, MBT_MAX_K = 16, MBT_MAX_SHIFTS = 4, MBT_NEWTON = 8, MBT_ADVECT_WALK = 64;

template <typename T>
struct MbtMesh {
    int N, NB, V, kv, kc, S;
    const int32_t* cell_vert;       // [N][2^d]
    const T* cell_xyz;              // [N][2^d][d]
    const int32_t* nbr;             // [2d][N]
    const uint8_t* fcode;           // [2d][N]
    const int32_t* vel_idx; const T* vel_w;         // [V][kv]
    const int32_t* cell_idx; const T* cell_w;       // [V][kc]
    T slack;
    T shift[MBT_MAX_SHIFTS][3];
    const T* vel; long long vel_stride;
    const T* bvel; long long bvel_stride, bvel_cs;
};

template <typename T>
struct MbtExtra {
    const T* field[MBT_MAX_EXTRA];
    long long stride[MBT_MAX_EXTRA];
};

template <typename T>
__device__ __forceinline__ T mbt_blend(T a, T b, T w) { return w == (T)1 ? b : a + w * (b - a); }

template <typename T>
__device__ __forceinline__ T mbt_clamp01(T x) { return x >= (T)0 ? (x <= (T)1 ? x : (T)1) : (T)0; }      // (a NaN becomes 0)

__device__ __forceinline__ int mbt_clamp_cell(int c, int N) { return min(max(c, 0), N - 1); }

template <typename T, int D>
__device__ __forceinline__ void mbt_load_corners(const MbtMesh<T>& m, int cell, T (&X)[1 << D][D]) {
    const T* p = m.cell_xyz + (long long)cell * ((1 << D) * D);
#pragma unroll
    for (int k = 0; k < (1 << D); ++k)
#pragma unroll
        for (int a = 0; a < D; ++a) X[k][a] = p[k * D + a];
}

// the cell map x(xi) and its Jacobian J[a][b] = d x_a / d xi_b
template <typename T, int D>
__device__ __forceinline__ void mbt_map(const T (&X)[1 << D][D], const T (&xi)[D], T (&x)[D], T (&J)[D][D]) {
#pragma unroll
    for (int a = 0; a < D; ++a) {
        if constexpr (D == 2) {
            const T e0 = mbt_blend(X[0][a], X[1][a], xi[0]), e1 = mbt_blend(X[2][a], X[3][a], xi[0]);
            x[a] = mbt_blend(e0, e1, xi[1]);
            J[a][0] = mbt_blend(X[1][a] - X[0][a], X[3][a] - X[2][a], xi[1]);
            J[a][1] = e1 - e0;
        } else {
            const T e0 = mbt_blend(X[0][a], X[1][a], xi[0]), e1 = mbt_blend(X[2][a], X[3][a], xi[0]);
            const T e2 = mbt_blend(X[4][a], X[5][a], xi[0]), e3 = mbt_blend(X[6][a], X[7][a], xi[0]);
            const T f0 = mbt_blend(e0, e1, xi[1]), f1 = mbt_blend(e2, e3, xi[1]);
            x[a] = mbt_blend(f0, f1, xi[2]);
            J[a][0] = mbt_blend(mbt_blend(X[1][a] - X[0][a], X[3][a] - X[2][a], xi[1]),
                                mbt_blend(X[5][a] - X[4][a], X[7][a] - X[6][a], xi[1]), xi[2]);
            J[a][1] = mbt_blend(e1 - e0, e3 - e2, xi[2]);
            J[a][2] = f1 - f0;
        }
    }
}

// Newton on the cell map from xi = 1/2
template <typename T, int D>
__device__ __forceinline__ void mbt_newton(const T (&X)[1 << D][D], const T (&p)[D], T slack, T (&xi)[D]) {
#pragma unroll
    for (int a = 0; a < D; ++a) xi[a] = (T)0.5;
    const T stop = slack / (T)4;
    for (int it = 0; it < MBT_NEWTON; ++it) {
        T x[D], J[D][D], r[D], dx[D];
        mbt_map<T, D>(X, xi, x, J);
#pragma unroll
        for (int a = 0; a < D; ++a) r[a] = x[a] - p[a];
        if constexpr (D == 2) {
            const T det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            dx[0] = (r[0] * J[1][1] - J[0][1] * r[1]) / det;
            dx[1] = (J[0][0] * r[1] - r[0] * J[1][0]) / det;
        } else {
            const T c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                    c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            const T det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
            const T c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2], c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0],
                    c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
            const T c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1], c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2],
                    c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            dx[0] = (c00 * r[0] + c10 * r[1] + c20 * r[2]) / det;       // (the inverse is the transposed cofactor matrix over det)
            dx[1] = (c01 * r[0] + c11 * r[1] + c21 * r[2]) / det;
            dx[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) / det;
        }
        bool small = true;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const T v = xi[a] - dx[a];
            xi[a] = v < (T)-1 ? (T)-1 : (v > (T)2 ? (T)2 : v);          // (a NaN passes through)
            small = small && FG_FABS(dx[a]) < stop;
        }
        if (small) break;
    }
}

// the walk: p (and q, a second position in the same periodic image, where given) are shifted at periodic faces; returns the status,
// xi clamped to [0, 1]^d, `slot` the boundary slot of status 1
template <typename T, int D>
__device__ __forceinline__ int mbt_walk(const MbtMesh<T>& m, T (&p)[D], T* q, int& cell, T (&xi)[D], int (&wr)[MBT_MAX_SHIFTS], int max_walk,
                                        int& slot) {
    int prev = -1, status = 2, changes = 0;
    bool accept = false;
    slot = 0;
    for (;;) {
        T X[1 << D][D], viol[2 * D];
        mbt_load_corners<T, D>(m, cell, X);
        mbt_newton<T, D>(X, p, m.slack, xi);
        bool inside = true, nan = false;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            viol[2 * a] = -xi[a];
            viol[2 * a + 1] = xi[a] - (T)1;
            inside = inside && xi[a] >= -m.slack && xi[a] <= (T)1 + m.slack;
            nan = nan || xi[a] != xi[a];
        }
        if (nan) break;
        if (inside || accept) { status = 0; break; }
        unsigned tried = 0;
        int next = -1, code = 0, first_slot = -1;
        for (int t = 0; t < 2 * D; ++t) {
            int best = -1;
            T bv = m.slack;
#pragma unroll
            for (int f = 0; f < 2 * D; ++f)
                if (!((tried >> f) & 1u) && viol[f] > bv) { bv = viol[f]; best = f; }
            if (best < 0) break;
            tried |= 1u << best;
            const int nb = m.nbr[(long long)best * m.N + cell];
            if (nb >= 0) { next = nb; code = (int)m.fcode[(long long)best * m.N + cell]; break; }
            if (first_slot < 0) first_slot = -1 - nb;
        }
        if (next < 0) { status = 1; slot = min(max(first_slot, 0), max(m.NB - 1, 0)); break; }
        if (changes >= max_walk) break;
        ++changes;
        if (code > 0) {
            const int s = min((code - 1) >> 1, MBT_MAX_SHIFTS - 1);
            const bool back = ((code - 1) & 1) != 0;        // odd codes: position -= shift, wraps += 1; even ones the reverse
#pragma unroll
            for (int k = 0; k < MBT_MAX_SHIFTS; ++k) {
                if (k != s) continue;
                wr[k] += back ? -1 : 1;
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    p[a] = back ? p[a] + m.shift[k][a] : p[a] - m.shift[k][a];
                    if (q) q[a] = back ? q[a] + m.shift[k][a] : q[a] - m.shift[k][a];
                }
            }
        }
        accept = next == prev;
        prev = cell;
        cell = mbt_clamp_cell(next, m.N);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) xi[a] = mbt_clamp01(xi[a]);
    return status;
}

// the velocity at (cell, xi): vertex values from the velocity stencils, then the blend
template <typename T, int D>
__device__ __forceinline__ void mbt_velocity(const MbtMesh<T>& m, const T* __restrict__ vel, const T* __restrict__ bvel, int cell,
                                             const T (&xi)[D], T (&u)[D]) {
    T val[1 << D][D];
#pragma unroll
    for (int k = 0; k < (1 << D); ++k) {
        const long long row = (long long)m.cell_vert[(long long)cell * (1 << D) + k] * m.kv;
#pragma unroll
        for (int a = 0; a < D; ++a) val[k][a] = (T)0;
        for (int j = 0; j < m.kv; ++j) {
            const T w = m.vel_w[row + j];
            if (w == (T)0) continue;
            const int idx = m.vel_idx[row + j];
            const T* src = idx < m.N ? vel + idx : bvel + (idx - m.N);
            const long long cs = idx < m.N ? (long long)m.N : m.bvel_cs;
#pragma unroll
            for (int a = 0; a < D; ++a) val[k][a] += w * src[a * cs];
        }
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const T e0 = mbt_blend(val[0][a], val[1][a], xi[0]), e1 = mbt_blend(val[2][a], val[3][a], xi[0]);
        if constexpr (D == 2) {
            u[a] = mbt_blend(e0, e1, xi[1]);
        } else {
            const T e2 = mbt_blend(val[4][a], val[5][a], xi[0]), e3 = mbt_blend(val[6][a], val[7][a], xi[0]);
            u[a] = mbt_blend(mbt_blend(e0, e1, xi[1]), mbt_blend(e2, e3, xi[1]), xi[2]);
        }
    }
}

// a cell-only field at (cell, xi)
template <typename T, int D>
__device__ __forceinline__ T mbt_scalar(const MbtMesh<T>& m, const T* __restrict__ f, int cell, const T (&xi)[D]) {
    T val[1 << D];
#pragma unroll
    for (int k = 0; k < (1 << D); ++k) {
        const long long row = (long long)m.cell_vert[(long long)cell * (1 << D) + k] * m.kc;
        val[k] = (T)0;
        for (int j = 0; j < m.kc; ++j) {
            const T w = m.cell_w[row + j];
            if (w == (T)0) continue;
            val[k] += w * f[m.cell_idx[row + j]];
        }
    }
    const T e0 = mbt_blend(val[0], val[1], xi[0]), e1 = mbt_blend(val[2], val[3], xi[0]);
    if constexpr (D == 2) {
        return mbt_blend(e0, e1, xi[1]);
    } else {
        const T e2 = mbt_blend(val[4], val[5], xi[0]), e3 = mbt_blend(val[6], val[7], xi[0]);
        return mbt_blend(mbt_blend(e0, e1, xi[1]), mbt_blend(e2, e3, xi[1]), xi[2]);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(MBT_BLOCK) void k_mb_point_locate(MbtMesh<T> m, const T* __restrict__ points, long long points_env_stride,
                                                               int n_points, const int32_t* __restrict__ start_cell, int max_walk,
                                                               int32_t* __restrict__ cell_out, T* __restrict__ xi_out,
                                                               int32_t* __restrict__ status_out) {
    const int i = (int)blockIdx.x * MBT_BLOCK + (int)threadIdx.x, env = (int)blockIdx.y;
    if (i >= n_points) return;
    const T* p = points + (long long)env * points_env_stride + (long long)i * D;
    T x[D], xi[D];
#pragma unroll
    for (int a = 0; a < D; ++a) x[a] = p[a];
    int wr[MBT_MAX_SHIFTS] = {0, 0, 0, 0}, slot;
    int cell = mbt_clamp_cell(start_cell[(long long)env * (points_env_stride / D) + i], m.N);
    const int status = mbt_walk<T, D>(m, x, nullptr, cell, xi, wr, max_walk, slot);
    const long long o = (long long)env * n_points + i;
    cell_out[o] = cell;
    status_out[o] = status;
#pragma unroll
    for (int a = 0; a < D; ++a) xi_out[o * D + a] = xi[a];
}

template <typename T, int D>
__global__ __launch_bounds__(MBT_BLOCK) void k_mb_point_sample(MbtMesh<T> m, MbtExtra<T> e, int n_extra, const int32_t* __restrict__ cell,
                                                               const T* __restrict__ xi_in, long long cell_env_stride, int n_points,
                                                               T* __restrict__ out) {
    const int i = (int)blockIdx.x * MBT_BLOCK + (int)threadIdx.x, env = (int)blockIdx.y;
    if (i >= n_points) return;
    const long long src = (long long)env * cell_env_stride + i;
    const int c = mbt_clamp_cell(cell[src], m.N);
    T xi[D], u[D];
#pragma unroll
    for (int a = 0; a < D; ++a) xi[a] = mbt_clamp01(xi_in[src * D + a]);
    mbt_velocity<T, D>(m, m.vel + (long long)env * m.vel_stride, m.bvel + (long long)env * m.bvel_stride, c, xi, u);
    T* o = out + ((long long)env * n_points + i) * (D + n_extra);
#pragma unroll
    for (int a = 0; a < D; ++a) o[a] = u[a];
#pragma unroll
    for (int k = 0; k < MBT_MAX_EXTRA; ++k)
        if (k < n_extra) o[D + k] = mbt_scalar<T, D>(m, e.field[k] + (long long)env * e.stride[k], c, xi);
}

template <typename T, int D>
__global__ __launch_bounds__(MBT_BLOCK) void k_mb_tracer_advect(MbtMesh<T> m, T dt, int substeps, const uint8_t* __restrict__ respawn_slots,
                                                                const T* __restrict__ seed_pos, const int32_t* __restrict__ seed_cell,
                                                                T* __restrict__ pos, int32_t* __restrict__ cell_io, T* __restrict__ age,
                                                                int32_t* __restrict__ wraps, uint32_t* __restrict__ lost, int n_tracers) {
    const int i = (int)blockIdx.x * MBT_BLOCK + (int)threadIdx.x, env = (int)blockIdx.y;
    if (i >= n_tracers) return;
    const long long t = (long long)env * n_tracers + i;
    const T* vel = m.vel + (long long)env * m.vel_stride;
    const T* bvel = m.bvel + (long long)env * m.bvel_stride;
    T x[D], seed[D], xi[D];
    int wr[MBT_MAX_SHIFTS] = {0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < D; ++a) { x[a] = pos[t * D + a]; seed[a] = seed_pos[t * D + a]; }
#pragma unroll
    for (int k = 0; k < MBT_MAX_SHIFTS; ++k)
        if (k < m.S) wr[k] = wraps[t * m.S + k];
    int cell = mbt_clamp_cell(cell_io[t], m.N);
    const int scell = mbt_clamp_cell(seed_cell[t], m.N);
    const T h = dt / (T)substeps, half = (T)0.5 * h;
    unsigned n_lost = 0;
    bool reborn = false, have = false;        // have: (cell, xi) is the location of x
    // what a located position means for the tracer: lost (status 2) or beyond a flagged face -> back to the seed; beyond another FIXED
    // face -> onto the face, the cell map at the clamped xi.  Returns whether (cell, xi) is the location of x afterwards.
    auto settle = [&](int status, int slot) -> bool {
        bool respawn = false;
        if (status == 2) {
            n_lost += 1u;
            respawn = true;
        } else if (status == 1) {
            if (respawn_slots[slot]) {
                respawn = true;
            } else {
                T X[1 << D][D], J[D][D];
                mbt_load_corners<T, D>(m, cell, X);
                mbt_map<T, D>(X, xi, x, J);
            }
        }
        if (respawn) {
            reborn = true;
            cell = scell;
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = seed[a];
#pragma unroll
            for (int k = 0; k < MBT_MAX_SHIFTS; ++k) wr[k] = 0;
        }
        return !respawn;
    };
    for (int s = 0; s < substeps && !reborn; ++s) {       // (a respawn ends the call for the tracer: it rests at its seed, age 0)
        int slot;
        if (!have) {                            // the first sub-step of a call: locate where the tracer is
            have = settle(mbt_walk<T, D>(m, x, nullptr, cell, xi, wr, MBT_ADVECT_WALK, slot), slot);
            if (!have) break;
        }
        T u[D], xs[D], xim[D];
        mbt_velocity<T, D>(m, vel, bvel, cell, xi, u);
        bool finite = true;
#pragma unroll
        for (int a = 0; a < D; ++a) { xs[a] = x[a] + half * u[a]; finite = finite && xs[a] - xs[a] == (T)0; }
        int cm = cell;
        int status = finite ? mbt_walk<T, D>(m, xs, x, cm, xim, wr, MBT_ADVECT_WALK, slot) : 2;
        if (status != 2) {
            mbt_velocity<T, D>(m, vel, bvel, cm, xim, u);
#pragma unroll
            for (int a = 0; a < D; ++a) { x[a] += h * u[a]; finite = finite && x[a] - x[a] == (T)0; }
            cell = cm;
            status = finite ? mbt_walk<T, D>(m, x, nullptr, cell, xi, wr, MBT_ADVECT_WALK, slot) : 2;
        }
        have = settle(status, slot);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) pos[t * D + a] = x[a];
#pragma unroll
    for (int k = 0; k < MBT_MAX_SHIFTS; ++k)
        if (k < m.S) wraps[t * m.S + k] = wr[k];
    cell_io[t] = cell;
    age[t] = reborn ? (T)0 : age[t] + dt;
    if (n_lost) atomicAdd(&lost[env], n_lost);
}

// what the three entry points check of the mesh record, and its device form
int mbt_check_mesh(const char* entry, const fg_mb_point_mesh* pm, MbtMesh<fg_real>& m) {
    const std::string e(entry);
    FG_REQUIRE(pm != nullptr, FG_ERR_INVALID_ARG, e + ": null mesh record");
    FG_REQUIRE(pm->dims == 2 || pm->dims == 3, FG_ERR_INVALID_ARG, e + ": dims must be 2 or 3");
    FG_REQUIRE(pm->batch >= 1 && pm->batch <= 65535, FG_ERR_INVALID_ARG, e + ": batch must be in 1..65535");
    FG_REQUIRE(pm->n_cells >= 1 && pm->n_cells <= (1 << 28), FG_ERR_INVALID_ARG, e + ": n_cells must be in 1..2^28");
    FG_REQUIRE(pm->n_slots >= 0 && pm->n_vertices >= 1, FG_ERR_INVALID_ARG, e + ": n_slots must not be negative, n_vertices positive");
    FG_REQUIRE((long long)pm->n_cells + pm->n_slots < (1LL << 31), FG_ERR_INVALID_ARG, e + ": n_cells + n_slots must fit 31 bits");
    FG_REQUIRE(pm->kv >= 1 && pm->kc >= 1, FG_ERR_INVALID_ARG, e + ": kv and kc must be positive");
    FG_REQUIRE(pm->kv <= MBT_MAX_K && pm->kc <= MBT_MAX_K, FG_ERR_UNSUPPORTED, e + ": stencils of more than 16 entries (kv, kc)");
    FG_REQUIRE(pm->n_shifts >= 0, FG_ERR_INVALID_ARG, e + ": n_shifts must not be negative");
    FG_REQUIRE(pm->n_shifts <= MBT_MAX_SHIFTS, FG_ERR_UNSUPPORTED, e + ": more than 4 periodic shift vectors");
    FG_REQUIRE(pm->cell_vert && pm->cell_xyz && pm->neighbors && pm->face_code, FG_ERR_INVALID_ARG, e + ": null cell table");
    FG_REQUIRE(pm->vel_idx && pm->vel_w && pm->cell_idx && pm->cell_w, FG_ERR_INVALID_ARG, e + ": null stencil table");
    FG_REQUIRE(pm->slack > 0 && pm->slack < (fg_real)0.25, FG_ERR_INVALID_ARG, e + ": slack must be in (0, 0.25)");
    for (int s = 0; s < pm->n_shifts; ++s)
        for (int a = 0; a < pm->dims; ++a)
            FG_REQUIRE(pm->shifts[3 * s + a] - pm->shifts[3 * s + a] == 0, FG_ERR_INVALID_ARG, e + ": a shift vector is not finite");
    FG_REQUIRE(pm->velocity != nullptr && pm->bvel != nullptr, FG_ERR_INVALID_ARG, e + ": null velocity or boundary-velocity pointer");
    FG_REQUIRE(pm->velocity_stride >= (long long)pm->dims * pm->n_cells, FG_ERR_INVALID_ARG, e + ": velocity stride smaller than dims * n_cells");
    FG_REQUIRE(pm->bvel_comp_stride >= pm->n_slots && pm->bvel_stride >= (long long)pm->dims * pm->bvel_comp_stride, FG_ERR_INVALID_ARG,
               e + ": boundary strides smaller than the slot array");
    m.N = pm->n_cells; m.NB = pm->n_slots; m.V = pm->n_vertices; m.kv = pm->kv; m.kc = pm->kc; m.S = pm->n_shifts;
    m.cell_vert = pm->cell_vert; m.cell_xyz = pm->cell_xyz; m.nbr = pm->neighbors; m.fcode = pm->face_code;
    m.vel_idx = pm->vel_idx; m.vel_w = pm->vel_w; m.cell_idx = pm->cell_idx; m.cell_w = pm->cell_w;
    m.slack = pm->slack;
    for (int s = 0; s < MBT_MAX_SHIFTS; ++s)
        for (int a = 0; a < 3; ++a) m.shift[s][a] = (s < pm->n_shifts && a < pm->dims) ? pm->shifts[3 * s + a] : (fg_real)0;
    m.vel = pm->velocity; m.vel_stride = pm->velocity_stride;
    m.bvel = pm->bvel; m.bvel_stride = pm->bvel_stride; m.bvel_cs = pm->bvel_comp_stride;
    return FG_OK;
}

}  // namespace

extern "C" int fg_mb_point_locate(const fg_mb_point_mesh* pm, const fg_real* points, int64_t points_env_stride, int32_t n_points,
                                  const int32_t* start_cell, int32_t max_walk, int32_t* cell_out, fg_real* xi_out, int32_t* status_out,
                                  void* stream) {
    MbtMesh<fg_real> m;
    if (int rc = mbt_check_mesh("fg_mb_point_locate", pm, m)) return rc;
    FG_REQUIRE(points && start_cell && cell_out && xi_out && status_out, FG_ERR_INVALID_ARG,
               "fg_mb_point_locate: null points, start_cell, cell_out, xi_out or status_out pointer");
    FG_REQUIRE(n_points >= 1, FG_ERR_INVALID_ARG, "fg_mb_point_locate: n_points must be at least 1");
    FG_REQUIRE(max_walk >= 0, FG_ERR_INVALID_ARG, "fg_mb_point_locate: max_walk must not be negative");
    FG_REQUIRE(points_env_stride == 0 || points_env_stride == (long long)n_points * pm->dims, FG_ERR_INVALID_ARG,
               "fg_mb_point_locate: the env stride of the points is 0 or n_points * dims");
    const dim3 grid((unsigned)((n_points + MBT_BLOCK - 1) / MBT_BLOCK), (unsigned)pm->batch);
    hipStream_t st = (hipStream_t)stream;
    if (pm->dims == 2)
        hipLaunchKernelGGL((k_mb_point_locate<fg_real, 2>), grid, dim3(MBT_BLOCK), 0, st, m, points, (long long)points_env_stride,
                           (int)n_points, start_cell, (int)max_walk, cell_out, xi_out, status_out);
    else
        hipLaunchKernelGGL((k_mb_point_locate<fg_real, 3>), grid, dim3(MBT_BLOCK), 0, st, m, points, (long long)points_env_stride,
                           (int)n_points, start_cell, (int)max_walk, cell_out, xi_out, status_out);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_mb_point_sample(const fg_mb_point_mesh* pm, const fg_real* const* extra, const int64_t* extra_stride, int32_t n_extra,
                                  const int32_t* cell, const fg_real* xi, int64_t cell_env_stride, int32_t n_points, fg_real* out,
                                  void* stream) {
    MbtMesh<fg_real> m;
    if (int rc = mbt_check_mesh("fg_mb_point_sample", pm, m)) return rc;
    FG_REQUIRE(cell && xi && out, FG_ERR_INVALID_ARG, "fg_mb_point_sample: null cell, xi or out pointer");
    FG_REQUIRE(n_points >= 1, FG_ERR_INVALID_ARG, "fg_mb_point_sample: n_points must be at least 1");
    FG_REQUIRE(n_extra >= 0 && n_extra <= MBT_MAX_EXTRA, FG_ERR_INVALID_ARG, "fg_mb_point_sample: n_extra must be in 0..8");
    FG_REQUIRE(n_extra == 0 || (extra != nullptr && extra_stride != nullptr), FG_ERR_INVALID_ARG, "fg_mb_point_sample: null extra tables");
    FG_REQUIRE(cell_env_stride == 0 || cell_env_stride >= n_points, FG_ERR_INVALID_ARG,
               "fg_mb_point_sample: the env stride of the cells is 0 or at least n_points");
    MbtExtra<fg_real> e;
    for (int k = 0; k < MBT_MAX_EXTRA; ++k) { e.field[k] = nullptr; e.stride[k] = 0; }
    for (int k = 0; k < n_extra; ++k) {
        FG_REQUIRE(extra[k] != nullptr, FG_ERR_INVALID_ARG, "fg_mb_point_sample: null extra field");
        FG_REQUIRE(extra_stride[k] >= pm->n_cells, FG_ERR_INVALID_ARG, "fg_mb_point_sample: an extra stride smaller than n_cells");
        e.field[k] = extra[k]; e.stride[k] = extra_stride[k];
    }
    const dim3 grid((unsigned)((n_points + MBT_BLOCK - 1) / MBT_BLOCK), (unsigned)pm->batch);
    hipStream_t st = (hipStream_t)stream;
    if (pm->dims == 2)
        hipLaunchKernelGGL((k_mb_point_sample<fg_real, 2>), grid, dim3(MBT_BLOCK), 0, st, m, e, (int)n_extra, cell, xi,
                           (long long)cell_env_stride, (int)n_points, out);
    else
        hipLaunchKernelGGL((k_mb_point_sample<fg_real, 3>), grid, dim3(MBT_BLOCK), 0, st, m, e, (int)n_extra, cell, xi,
                           (long long)cell_env_stride, (int)n_points, out);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_mb_tracer_advect(const fg_mb_point_mesh* pm, fg_real dt, int32_t substeps, const uint8_t* respawn_slots,
                                   const fg_real* seed_pos, const int32_t* seed_cell, fg_real* pos, int32_t* cell, fg_real* age,
                                   int32_t* wraps, uint32_t* lost, int32_t n_tracers, void* stream) {
    MbtMesh<fg_real> m;
    if (int rc = mbt_check_mesh("fg_mb_tracer_advect", pm, m)) return rc;
    FG_REQUIRE(respawn_slots && seed_pos && seed_cell && pos && cell && age && lost, FG_ERR_INVALID_ARG,
               "fg_mb_tracer_advect: null respawn_slots, seed_pos, seed_cell, pos, cell, age or lost pointer");
    FG_REQUIRE(pm->n_shifts == 0 || wraps != nullptr, FG_ERR_INVALID_ARG, "fg_mb_tracer_advect: null wraps pointer on a periodic mesh");
    FG_REQUIRE(substeps >= 1, FG_ERR_INVALID_ARG, "fg_mb_tracer_advect: substeps must be at least 1");
    FG_REQUIRE(n_tracers >= 1, FG_ERR_INVALID_ARG, "fg_mb_tracer_advect: n_tracers must be at least 1");
    FG_REQUIRE(dt - dt == 0, FG_ERR_INVALID_ARG, "fg_mb_tracer_advect: dt must be finite");
    const dim3 grid((unsigned)((n_tracers + MBT_BLOCK - 1) / MBT_BLOCK), (unsigned)pm->batch);
    hipStream_t st = (hipStream_t)stream;
    if (pm->dims == 2)
        hipLaunchKernelGGL((k_mb_tracer_advect<fg_real, 2>), grid, dim3(MBT_BLOCK), 0, st, m, dt, (int)substeps, respawn_slots, seed_pos,
                           seed_cell, pos, cell, age, wraps, lost, (int)n_tracers);
    else
        hipLaunchKernelGGL((k_mb_tracer_advect<fg_real, 3>), grid, dim3(MBT_BLOCK), 0, st, m, dt, (int)substeps, respawn_slots, seed_pos,
                           seed_cell, pos, cell, age, wraps, lost, (int)n_tracers);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}
