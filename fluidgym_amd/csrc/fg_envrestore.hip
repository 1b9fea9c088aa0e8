// Per-env restore: chosen envs of the batch become states of a bank, each with its own mirror and roll along the periodic axes
// (the per-env form of the reference's batch-wide randomisation, rbc_env_base.py:335-362: torch.flip, the sign of the mirrored
// velocity component, torch.roll).  One launch per field; the grid runs over (selected env, tile), never over the whole batch, and
// an env that is not named is not written.  Every value is a copy or a negation, so the result is bit-exact.
//
// Shape: a field is rows of ex cells, row = (c, z, y).  A workgroup of 64 x 4 threads covers 64 cells of 16 rows in four passes, one
// cell per lane: every store instruction of a wave writes 256 contiguous bytes (fp32) of one row; the mirrored / rolled read is the
// same row segment backwards, or two segments either side of the wrap.  The selection record is read once per workgroup through a
// wave-uniform address.  No atomics, no data-dependent loop, nothing returns to the host.
#include <vector>

#include "fg_internal.h"

namespace {

constexpr int ER_TX = 64, ER_TY = 4, ER_PASSES = 4, ER_ROWS = ER_TY * ER_PASSES;

template <typename T>
__global__ __launch_bounds__(ER_TX * ER_TY) void k_env_restore(T* __restrict__ dst, const T* __restrict__ bank,
                                                               const fg_env_sel* __restrict__ sel, int C, int ez, int ey, int ex,
                                                               int tiles_x, int signed_components) {
    const fg_env_sel r = sel[blockIdx.y];
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), rg = (int)(blockIdx.x / (unsigned)tiles_x);
    const int rows = C * ez * ey;
    const size_t per_env = (size_t)rows * ex;
    T* __restrict__ d = dst + (size_t)r.env * per_env;
    const T* __restrict__ b = bank + (size_t)r.src * per_env;
    const int x = tx * ER_TX + (int)threadIdx.x;
    int xs = x - r.shift_x;
    if (xs < 0) xs += ex;
    if (r.flip_x) xs = ex - 1 - xs;
#pragma unroll
    for (int k = 0; k < ER_PASSES; ++k) {
        const int row = rg * ER_ROWS + k * ER_TY + (int)threadIdx.y;
        if (x < ex && row < rows) {
            const int y = row % ey, cz = row / ey;
            const int z = cz % ez, c = cz / ez;
            int zs = z - r.shift_z;
            if (zs < 0) zs += ez;
            if (r.flip_z) zs = ez - 1 - zs;
            const T v = b[((size_t)(c * ez + zs) * ey + y) * ex + xs];
            const bool neg = signed_components && ((c == 0 && r.flip_x) || (c == 2 && r.flip_z));
            d[(size_t)row * ex + x] = neg ? -v : v;
        }
    }
}

// the chosen envs' slice of velocityResult := block velocity [d n], of pressureResult := 0 [n]; four cells per thread
template <typename T>
__global__ __launch_bounds__(256) void k_env_reset_solver(const T* __restrict__ velocity, T* __restrict__ vel_result,
                                                          T* __restrict__ p_result, const fg_env_sel* __restrict__ sel, long n, int dims) {
    const int env = sel[blockIdx.y].env;
    const long dn = (long)dims * n;
    const T* __restrict__ u = velocity + (size_t)env * dn;
    T* __restrict__ ur = vel_result + (size_t)env * dn;
    T* __restrict__ pr = p_result + (size_t)env * n;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = ((long)blockIdx.x * 4 + k) * 256 + threadIdx.x;
        if (i < dn) ur[i] = u[i];
        if (i < n) pr[i] = (T)0;
    }
}

// what every entry checks of the records that name envs: count, range, no env twice
int check_envs(const fg_state* s, const fg_env_sel* sel, int32_t n_sel, const char* who) {
    const int B = s->grid.B;
    FG_REQUIRE(sel != nullptr, FG_ERR_INVALID_ARG, std::string(who) + ": null selection");
    FG_REQUIRE(n_sel >= 1 && n_sel <= B, FG_ERR_INVALID_ARG, std::string(who) + ": n_sel must be in 1..batch");
    FG_REQUIRE(n_sel <= 65535, FG_ERR_UNSUPPORTED, std::string(who) + ": at most 65535 envs per call");
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n_sel; ++i) {
        FG_REQUIRE(sel[i].env >= 0 && sel[i].env < B, FG_ERR_INVALID_ARG, std::string(who) + ": env index out of range");
        FG_REQUIRE(!seen[sel[i].env], FG_ERR_INVALID_ARG, std::string(who) + ": an env is named twice");
        seen[sel[i].env] = 1;
    }
    return FG_OK;
}

}  // namespace

extern "C" int fg_env_restore_field(fg_handle s, int which_field, const fg_real* bank, int32_t S, const fg_env_sel* sel, int32_t n_sel,
                                    int32_t signed_components, void* stream) {
    FG_REQUIRE(s != nullptr, FG_ERR_INVALID_ARG, "fg_env_restore_field: null handle");
    FG_REQUIRE(bank != nullptr && S >= 1, FG_ERR_INVALID_ARG, "fg_env_restore_field: null bank or S < 1");
    if (int rc = check_envs(s, sel, n_sel, "fg_env_restore_field")) return rc;
    const FgGrid& g = s->grid;
    // the field: destination, components, vector or not, extents (a face array has extent 1 along its normal axis)
    fg_real* dst = nullptr;
    int C = 0, vector_field = 0, ext[3] = {g.nx, g.ny, g.nz};
    if (which_field == FG_VELOCITY) { dst = s->velocity; C = g.dims; vector_field = 1; }
    else if (which_field == FG_PRESSURE) { dst = s->pressure; C = 1; }
    else if (which_field == FG_SCALAR) { dst = s->scalar; C = s->cfg.n_scalars; }
    else if (which_field == FG_VELOCITY_SOURCE) { dst = s->velocity_source; C = g.dims; vector_field = 1; }
    else if (which_field >= FG_BOUND_VELOCITY && which_field < FG_BOUND_VELOCITY + 2 * g.dims) {
        const int f = which_field - FG_BOUND_VELOCITY;
        dst = s->bvel[f]; C = g.dims; vector_field = 1; ext[f >> 1] = 1;
    } else if (which_field >= FG_BOUND_SCALAR && which_field < FG_BOUND_SCALAR + 2 * g.dims) {
        const int f = which_field - FG_BOUND_SCALAR;
        dst = s->bscal[f]; C = s->cfg.n_scalars; ext[f >> 1] = 1;
    } else FG_REQUIRE(false, FG_ERR_INVALID_ARG, "fg_env_restore_field: unknown field id");
    FG_REQUIRE(signed_components == 0 || (signed_components == 1 && vector_field), FG_ERR_INVALID_ARG,
               "fg_env_restore_field: signed_components is 0, or 1 on a vector field");
    const bool x_periodic = !g.fixed[0] && !g.fixed[1], z_periodic = g.dims == 3 && !g.fixed[4] && !g.fixed[5];
    for (int i = 0; i < n_sel; ++i) {
        const fg_env_sel& r = sel[i];
        FG_REQUIRE(r.src >= 0 && r.src < S, FG_ERR_INVALID_ARG, "fg_env_restore_field: src index out of range");
        FG_REQUIRE((r.flip_x | 1) == 1 && (r.flip_z | 1) == 1, FG_ERR_INVALID_ARG, "fg_env_restore_field: a flip is 0 or 1");
        FG_REQUIRE(g.dims == 3 || (r.flip_z == 0 && r.shift_z == 0), FG_ERR_INVALID_ARG, "fg_env_restore_field: flip_z / shift_z on a 2-D grid");
        FG_REQUIRE(r.shift_x >= 0 && r.shift_x < g.nx && r.shift_z >= 0 && r.shift_z < g.nz, FG_ERR_INVALID_ARG,
                   "fg_env_restore_field: a shift must be in [0, n)");
        FG_REQUIRE(x_periodic || (r.flip_x == 0 && r.shift_x == 0), FG_ERR_INVALID_ARG, "fg_env_restore_field: flip / shift along x, which has FIXED faces");
        FG_REQUIRE(g.dims == 2 || z_periodic || (r.flip_z == 0 && r.shift_z == 0), FG_ERR_INVALID_ARG,
                   "fg_env_restore_field: flip / shift along z, which has FIXED faces");
    }
    FG_REQUIRE(dst != nullptr && C > 0, FG_ERR_NOT_BOUND, "fg_env_restore_field: the field is not bound");
    hipStream_t st = (hipStream_t)stream;
    FG_HIP_CHECK(hipMemcpyAsync(s->env_sel_dev, sel, sizeof(fg_env_sel) * n_sel, hipMemcpyHostToDevice, st));
    const int ex = ext[0], ey = ext[1], ez = ext[2];
    const int tiles_x = (ex + ER_TX - 1) / ER_TX;
    const long row_groups = ((long)C * ez * ey + ER_ROWS - 1) / ER_ROWS;
    hipLaunchKernelGGL(k_env_restore<fg_real>, dim3((unsigned)(tiles_x * row_groups), (unsigned)n_sel), dim3(ER_TX, ER_TY), 0, st, dst, bank,
                       (const fg_env_sel*)s->env_sel_dev, C, ez, ey, ex, tiles_x, (int)signed_components);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_env_reset_solver_state(fg_handle s, const fg_env_sel* sel, int32_t n_sel, void* stream) {
    FG_REQUIRE(s != nullptr, FG_ERR_INVALID_ARG, "fg_env_reset_solver_state: null handle");
    if (int rc = check_envs(s, sel, n_sel, "fg_env_reset_solver_state")) return rc;
    FG_REQUIRE(s->velocity != nullptr, FG_ERR_NOT_BOUND, "velocity not bound");
    hipStream_t st = (hipStream_t)stream;
    FG_HIP_CHECK(hipMemcpyAsync(s->env_sel_dev, sel, sizeof(fg_env_sel) * n_sel, hipMemcpyHostToDevice, st));
    const long n = s->grid.n, dn = n * s->grid.dims;
    hipLaunchKernelGGL(k_env_reset_solver<fg_real>, dim3((unsigned)((dn + 1023) / 1024), (unsigned)n_sel), dim3(256), 0, st,
                       (const fg_real*)s->velocity, s->vel_result, s->p_result, (const fg_env_sel*)s->env_sel_dev, n, s->grid.dims);
    FG_HIP_CHECK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_mb_env_restore_field(fg_mb_handle, int, const fg_real*, int32_t, const fg_env_sel*, int32_t, int32_t, void*) {
    fg_set_error("fg_mb_env_restore_field: a multi-block handle has no per-env restore");
    return FG_ERR_UNSUPPORTED;
}

extern "C" int fg_mb_env_reset_solver_state(fg_mb_handle, const fg_env_sel*, int32_t, void*) {
    fg_set_error("fg_mb_env_reset_solver_state: a multi-block handle has no per-env restore");
    return FG_ERR_UNSUPPORTED;
}
