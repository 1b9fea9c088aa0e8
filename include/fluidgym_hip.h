/*
 * fluidgym_hip.h -- C ABI of libfluidgym_hip.so, the MI355X (gfx950) native replacement for the
 * simulation hot path of safe-autonomous-systems/fluidgym (module `PISOtorch`,
 * reference: src/fluidgym/simulation/extensions/PISOtorch.cpp:40-670).
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / scalars (no torch types),
 * returns an int status (FG_OK = 0, negative = error, never aborts -- the reference `exit(10)`s on a
 * CUDA error, PISO_multiblock_cuda_kernel.cu:40-46) and is asynchronous on the `stream` it is
 * given (a hipStream_t passed as void*; the reference synchronises the device around every kernel,
 * PISO_multiblock_cuda_kernel.cu:4512,4520).  All `float*` arguments are DEVICE pointers unless
 * the name ends in `_host`.
 *
 * Differences from the reference object model:
 *   - an ENV BATCH axis B is the outermost axis of every field (the reference asserts N == 1,
 *     domain_structs.cpp:2020); per-env time steps are a device array dt[B]; dt[b] <= 0 marks env b
 *     inactive for that call (its state is left untouched);
 *   - one block, rectilinear (tensor-product) orthogonal grid: metrics are per-axis cell widths;
 *     faces are PERIODIC or FIXED (Dirichlet velocity; Dirichlet/Neumann passive scalar);
 *   - matrices are never materialised as CSR: C is kept in stencil form (diag + 2d off-diagonals),
 *     P is applied matrix-free from 1/A;
 *   - the caller owns all field memory and binds it with fg_bind(); the handle owns solver
 *     workspace allocated once in fg_create() -- nothing is allocated on the step path.
 *
 * Layouts (fp32, C-contiguous): velocity [B,d,(Z,)Y,X]; pressure [B,1,(Z,)Y,X];
 * passive scalar [B,C,(Z,)Y,X]; velocity source [B,d,(Z,)Y,X]; boundary velocity of face f
 * [B,d,slab(f)] and boundary scalar [B,C,slab(f)] where slab(f) is the cell shape with extent 1
 * on the face axis.  Faces: 0..5 = -x,+x,-y,+y,-z,+z (PISO_multiblock_cuda_kernel.cu:211-236).
 */
#ifndef FLUIDGYM_HIP_H
#define FLUIDGYM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 1

/* Scalar type of the fields, metrics and real-valued arguments of the SINGLE-BLOCK entry points (fg_create .. fg_poisson_fdcg).
 * libfluidgym_hip.so is built with fg_real = float (the reference's default dtype, envs/fluid_env.py:146);
 * libfluidgym_hip_f64.so is the same sources built with -DFG_REAL_DOUBLE: fg_real = double, for FluidEnv(dtype=torch.float64)
 * (assembly, BiCGStab, CG and the step drivers; the fp32-only fast-diagonalisation / z-marching / line-preconditioner kernels and
 * the multi-block path are not part of that build and their entry points return FG_ERR_UNSUPPORTED or are absent). */
#ifdef FG_REAL_DOUBLE
typedef double fg_real;
#else
typedef float fg_real;
#endif
#define FG_MAX_SCALARS 4

/* status codes */
#define FG_OK 0
#define FG_ERR_INVALID_ARG (-1)
#define FG_ERR_NOT_BOUND (-2)
#define FG_ERR_HIP (-3)
#define FG_ERR_UNSUPPORTED (-4)
#define FG_ERR_NOT_CONVERGED (-5) /* informational: a solve hit max_iterations */
#define FG_ERR_NOT_FINITE (-6)   /* a solver residual became NaN/Inf */
#define FG_ERR_FLUX_BALANCE (-7) /* |sum of boundary fluxes| > flux_balance_tol (simulation.py:223-231) */

/* boundary type of a face (reference BoundaryType::PERIODIC / FIXED, domain_structs_gpu.h:120-135) */
#define FG_PERIODIC 0
#define FG_FIXED 1
/* passive-scalar boundary condition (reference BoundaryConditionType) */
#define FG_DIRICHLET 0
#define FG_NEUMANN 1

/* bindable fields (fg_bind) */
enum fg_field {
    FG_VELOCITY = 0,       /* block.velocity           [B,d,N]                      */
    FG_PRESSURE = 1,       /* block.pressure           [B,N]                        */
    FG_SCALAR = 2,         /* block.passiveScalar      [B,C,N]                      */
    FG_VELOCITY_SOURCE = 3,/* block.velocitySource     [B,d,N] (NULL = none)        */
    FG_VISCOSITY_FIELD = 4,/* block.viscosity          [B,N] per-cell viscosity of the velocity system (NULL = the global one): Block.setViscosity
                              of the reference's SGS hook (tcf_env.py:441-474; getViscosityBlock, PISO_multiblock_cuda_kernel.cu:1816-1837) */
    FG_BOUND_VELOCITY = 8, /* + face: FixedBoundary.velocity      [B,d,slab]        */
    FG_BOUND_SCALAR = 16   /* + face: FixedBoundary.passiveScalar [B,C,slab]        */
};

/* pressure solver variants (the reference only has CG, cg_solver_kernel.cu:129-471) */
#define FG_SOLVER_CG 0
#define FG_SOLVER_JACOBI 1
#define FG_SOLVER_RBGS 2
#define FG_SOLVER_MGCG 3   /* reserved */
#define FG_SOLVER_FDCG 4   /* CG preconditioned by the separable constant-coefficient operator (fast diagonalisation) */

typedef struct fg_state* fg_handle;

typedef struct fg_config {
    int32_t dims;                 /* 2 or 3 */
    int32_t nx, ny, nz;           /* cells; nz = 1 in 2-D; >= 3 per used axis (domain_structs.cpp:1193) */
    int32_t batch;                /* B */
    int32_t n_scalars;            /* passive scalar channels C (0..FG_MAX_SCALARS) */
    int32_t face_type[6];         /* FG_PERIODIC / FG_FIXED; a FIXED face needs a FIXED partner */
    int32_t scalar_bc[6][FG_MAX_SCALARS]; /* FG_DIRICHLET / FG_NEUMANN per FIXED face & channel */
    int32_t device;               /* HIP device ordinal */
} fg_config;

/* result of a batched linear solve, one entry per system (reference LinearSolverResultInfo,
 * bicgstab_solver.h) */
typedef struct fg_solve_info {
    float final_residual;   /* RMS residual ||r||_2/sqrt(n) (cg_solver_kernel.cu:100-106) */
    int32_t used_iterations;
    int32_t converged;
    int32_t is_finite;
} fg_solve_info;

/* ---- lifetime ------------------------------------------------------------------------------ */
int fg_abi_version(void);
const char* fg_last_error(void);                 /* thread-local message of the last failure */

/* Domain()+CreateBlock()+PrepareSolve() (PISOtorch.cpp:420-500; domain_structs.cpp:2570-2693).
 * hx/hy/hz_host: per-axis cell widths (host arrays of nx/ny/nz floats; hz may be NULL in 2-D). */
int fg_create(const fg_config* cfg, const fg_real* hx_host, const fg_real* hy_host, const fg_real* hz_host,
              fg_handle* out);
int fg_destroy(fg_handle h);

/* Block.setVelocity()/setPressure()/... + Domain.UpdateDomainData() (domain_structs.cpp:3047-3283):
 * bind (borrow) a caller-owned device buffer.  field = enum fg_field (+ face for boundaries). */
int fg_bind(fg_handle h, int field, fg_real* ptr);
/* Domain.viscosity / Domain.setScalarViscosity (domain_structs.cpp:3070) */
int fg_set_viscosity(fg_handle h, fg_real viscosity);
int fg_set_scalar_viscosity(fg_handle h, int channel, fg_real viscosity);
/* One viscosity / scalar diffusivity PER ENV of the batch (no reference counterpart: its Domain holds one value).  nu_B / k_B:
 * caller-owned device array [batch], bound like dt_B -- every kernel that needs the value reads entry b at launch (one
 * wave-uniform load per workgroup), so the values may be rewritten between steps without a call or a host round trip.  NULL
 * returns to the scalar of fg_set_viscosity / fg_set_scalar_viscosity.  A scalar channel without an array of its own follows
 * the rule of the scalars (its own value once any channel was set, else the velocity's -- array included).  With a per-cell
 * FG_VISCOSITY_FIELD bound the field wins for the velocity system; the arrays still apply to the scalars.  The Helmholtz
 * preconditioner (fg_set_fd_helmholtz) factorises with env b's own diffusivity. */
int fg_set_viscosity_batch(fg_handle h, const fg_real* nu_B);
int fg_set_scalar_viscosity_batch(fg_handle h, int channel, const fg_real* k_B);

/* Fast-diagonalisation preconditioner factors for FG_SOLVER_FDCG (host arrays, copied to the device):
 * Qx [nx,nx] / QxT: H-orthonormal eigenbasis of the 1-D x operator and its transpose, Qz / QzT the same
 * for z (NULL in 2-D), lower [ny]: sub-diagonal of the y operator, inv / cp [(nz,) ny, nx]: per-mode
 * reciprocal pivots and modified super-diagonal of the tridiagonal LU along y.  Built by
 * fluidgym_amd/simulation/fd_precond.py; requires FIXED y faces.  No reference counterpart (the
 * reference runs un-preconditioned CG, cg_solver_kernel.cu:129-471). */
int fg_set_fd_preconditioner(fg_handle h, const float* Qx_host, const float* QxT_host, const float* Qz_host,
                             const float* QzT_host, const float* lower_host, const float* inv_host,
                             const float* cp_host);
/* Marks the x axis as a cosine-transform axis: uniform cell width `cell_width`, FIXED faces, nx in {64, 128, 256, 512}.
 * The caller must have passed the orthonormal DCT-II basis / sqrt(cell_width) (modes in DCT order) as Qx to
 * fg_set_fd_preconditioner; the library then applies it as one FFT per row (csrc/fg_fdfft.hip) instead of a dense
 * GEMM.  Returns FG_ERR_UNSUPPORTED for other lengths / axes (the GEMM path stays in place). */
int fg_set_fd_fast_transform(fg_handle h, int axis, float cell_width);
/* returnBestResult of the pressure CG (SolveLinear(..., returnBestResult), cg_solver_kernel.cu:345-361): on (default), a
 * solve that ends unconverged hands back the best iterate it kept (within 2x of the lowest residual reached) instead
 * of the last one; off saves the occasional extra store pass over x. */
int fg_set_return_best(fg_handle h, int on);
/* residualResetSteps of the pressure CG (SolveLinear(..., residualResetSteps), cg_solver_kernel.cu:281-302): every `steps`
 * iterations the residual is recomputed from the iterate, r = b - P x, and the recurrence restarts from it.  Default 100, the value
 * the reference's non-orthogonal branch passes (PISOtorch_simulation.py:1913); 0 = never. */
int fg_set_cg_reset_steps(fg_handle h, int steps);
/* Start vector of the velocity (advection) solve.  The reference's split step has two rules (recorded from its own Python in
 * tests/golden/reference_split_step.json): its orthogonal branch starts from velocityResult (advect_use_prev_result,
 * PISOtorch_simulation.py:1689-1693), its non-orthogonal branch -- which its TCF env also runs on a rectilinear grid
 * (tcf_env.py:497) -- from zero on the first non-orthogonal pass (x=None, :1735-1742).  from_result 1 (default of a new handle): the
 * orthogonal-branch rule; 0: zero.  Same converged answer within the tolerance, different iteration counts. */
int fg_set_advection_start(fg_handle h, int from_result);
/* Native form of the turbulent-channel env's PRE hook (tcf_env.py "dynamic forcing", grid.py:147-176): before every PISO step a
 * uniform body force along `axis`, per env  G = 1/2 (coef_lo <u_axis>_lo + coef_hi <u_axis>_hi), the means taken over the cell
 * layers next to the -y / +y walls (coef = nu / wall distance of the layer: the two wall shear stresses), is added to the velocity
 * right-hand side as a velocity source of that value would be.  axis < 0 switches it off.  Needs FIXED y faces. */
int fg_set_wall_stress_forcing(fg_handle h, int axis, fg_real coef_lo, fg_real coef_hi);

/* ---- reductions used by the drivers --------------------------------------------------------- */
/* Domain.getMaxVelocity(withBounds=True, computational=True) (domain_structs.cpp:1580-1611) */
int fg_max_velocity(fg_handle h, fg_real* out_B, void* stream);
/* Domain.GetBoundaryFluxBalance (domain_structs.cpp:2476-2509) */
int fg_boundary_flux_balance(fg_handle h, fg_real* out_B, void* stream);

/* Both reductions with ONE device->host transfer and one stream sync: out_host[0..B) = flux balance,
 * out_host[B..2B) = max velocity (what Simulation.single_step + _PISO_adaptive_step read per substep,
 * simulation.py:223-231 and PISOtorch_simulation.py:2013-2014). */
int fg_step_diagnostics(fg_handle h, fg_real* out_host_2B, void* stream);
/* update_advective_boundaries for one FIXED face with characteristic velocity velm (host, d floats)
 * (PISOtorch_simulation.py:282-389); envs with dt_B[b] <= 0 are skipped. */
int fg_update_advective_boundary(fg_handle h, int face, const fg_real* velm_host, const fg_real* dt_B, void* stream);
/* balance_boundary_fluxes (PISOtorch_simulation.py:188-224): free_face_mask bit f = face f is free. */
int fg_balance_boundary_fluxes(fg_handle h, int free_face_mask, fg_real atol, const fg_real* dt_B, void* stream);

/* ---- PISO building blocks (one call = the reference free function of the same role) --------- */
/* SetupAdvectionMatrix (PISO_multiblock_cuda_kernel.cu:4525-4546, kernel :3616-3880) fused with
 * SetupAdvectionVelocity (:4692-4708, kernel :4296-4400) or, when for_scalar != 0, with
 * SetupAdvectionScalar (:4620-4637, kernel :4094-4198) for `channel`. */
int fg_setup_advection(fg_handle h, const fg_real* dt_B, int for_scalar, int channel, void* stream);
/* SolveLinear(C, RHS, x, useBiCG=True) (:7085-7118; bicgstab_solver_kernel.cu:63-411) for the
 * velocity components (for_scalar = 0; x0 = previous velocityResult) or a scalar channel.
 * info_host: d (or 1) * B entries, written after an internal stream sync. */
int fg_solve_advection(fg_handle h, int for_scalar, int channel, fg_real tol, int max_iterations,
                       fg_solve_info* info_host, void* stream);
/* Preconditioner policy of the advection-diffusion solves (scalar and velocity), the reference's preconditionBiCG /
 * BiCG_precondition_fallback (PISOtorch_simulation.py:503, 565; PISOtorch_diff.py:449-476; cuSPARSE ILU(0),
 * bicgstab_solver_kernel.cu:191-226, 288-293): mode 0 = plain BiCGStab (the reference's first rung, default), 1 = every solve
 * right-preconditioned, 2 = a solve that ends unconverged or non-finite is repeated from zero with the preconditioner.  The
 * preconditioner of modes 1 / 2 is the tridiagonal part of the matrix along y (csrc/fg_linepre.hip), factorised per solve and env;
 * 3 = every solve preconditioned by the separable Helmholtz operator (fg_set_fd_helmholtz); 4 / 5 = like 1 / 2 with the reference's
 * own preconditioner, ILU(0) of the matrix (csrc/fg_ilu0.hip: closed form on the stencil, hyperplane sweeps; every axis >= 4 cells).
 * fg_advection_retries: number of repeated solves since the last reset. */
int fg_set_advection_preconditioner(fg_handle h, int mode);
/* SGSviscosityIncompressibleSmagorinsky (PISO_multiblock_cuda_kernel.cu:6913-6966): out[B,N] = coefficient * Delta^2 * |S| with
 * |S| = sqrt(2 S:S) from the gradients of the bound velocity (getBlockDataGradient, :2997-3040: central differences, a Dirichlet face
 * counts as half a cell) and Delta^2 = the largest squared cell extent.  Asynchronous on `stream`. */
int fg_sgs_smagorinsky(fg_handle h, fg_real coefficient, fg_real* out_BN, void* stream);
/* Velocity-gradient diagnostics of the bound velocity (ComputeSpatialVelocityGradients = getBlockDataGradient per component,
 * PISO_multiblock_cuda_kernel.cu:2997-3040, 6460-6553; csrc/fg_flowdiag.hip): out[B, K, (nz,) ny, nx], one launch over the whole batch,
 * asynchronous on `stream`, nothing returns to the host, the bound fields are only read.  With g[i][j] = d u_i / d x_j (central
 * differences of the neighbour values, a Dirichlet face counts as half a cell, times Minv), S = sym(g), Omega = skew(g), d = dims:
 *   FG_DIAG_GRADIENT             K = d d   g[i][j] in channel i d + j
 *   FG_DIAG_VORTICITY            K = 1 (2-D): g[1][0] - g[0][1];  K = 3 (3-D): (g[2][1] - g[1][2], g[0][2] - g[2][0], g[1][0] - g[0][1])
 *   FG_DIAG_VORTICITY_MAGNITUDE  K = 1     its Euclidean norm (absolute value in 2-D)
 *   FG_DIAG_Q                    K = 1     0.5 (|Omega|^2 - |S|^2), Frobenius norms
 *   FG_DIAG_STRAIN_NORM          K = 1     sqrt(2 S:S), the |S| of fg_sgs_smagorinsky
 * Before any launch: FG_ERR_INVALID_ARG for a null handle or out or an unknown kind, FG_ERR_NOT_BOUND when the velocity (or the
 * boundary velocity of a FIXED face) is not bound. */
#define FG_DIAG_GRADIENT 0
#define FG_DIAG_VORTICITY 1
#define FG_DIAG_VORTICITY_MAGNITUDE 2
#define FG_DIAG_Q 3
#define FG_DIAG_STRAIN_NORM 4
int fg_flow_diagnostic(fg_handle h, int kind, fg_real* out, void* stream);
/* Test / diagnosis entry, never on a step path: z = M^-1 r [B, nc, N] with the preconditioner of `mode` (1: y-line, 3: the separable
 * Helmholtz operator of the velocity system, I/dt - nu Laplacian with the dt of the last velocity fg_setup_advection, applied by the
 * dispatch the BiCGStab runs; 4: ILU(0)) built from the advection-diffusion matrix currently assembled (fg_setup_advection).
 * forms_out (optional): int32_t[FG_FORM_SLOTS], the kernel forms that ran (FG_FORM_* below).  Synchronises. */
int fg_debug_apply_preconditioner(fg_handle h, int mode, int nc, const fg_real* r, fg_real* z, int32_t* forms_out, void* stream);
/* Test / diagnosis entry, never on a step path: z = M^-1 r [B, N] with a preconditioner of the pressure CG, run by the dispatch the
 * solvers run on this grid.  form 0: the grid's A = 1 operator (fg_fd_apply, with its fused r.z); 1: the row-mean operator (1/A replaced
 * by its mean along x per row and env), factors made from rA [B, N] by their own launch; 2: the same operator with the factors made
 * inside the tridiagonal launch from the per-tile row sums the last velocity fg_setup_advection left (rA must be nullptr: that
 * assembly's 1/A).  rz_out (optional, host): double[B], r.z per env.  forms_out (optional): int32_t[FG_FORM_SLOTS].  A form the grid
 * or the build does not carry returns FG_ERR_UNSUPPORTED with its reason (forms 1 / 2: 2-D, fast x transform, nx % 64 == 0,
 * ny <= 320; form 2 also the LDS of the factoring launch; the fp64 build carries form 0 only).  Synchronises. */
int fg_debug_apply_pressure_preconditioner(fg_handle h, int form, const fg_real* rA, const fg_real* r, fg_real* z, double* rz_out,
                                           int32_t* forms_out, void* stream);
/* forms_out of the two entries above: slot -> the form of that step of the application (0 = the step did not run) */
#define FG_FORM_SLOTS 8
#define FG_FORM_SLOT_X 0          /* x basis change */
#define FG_FORM_SLOT_Z 1          /* z basis change (3-D) */
#define FG_FORM_SLOT_TRIDIAG 2    /* per-mode tridiagonal solve of the pressure operator */
#define FG_FORM_SLOT_FACTORS 3    /* the factors that solve used */
#define FG_FORM_SLOT_HELM 4       /* Helmholtz per-mode solve */
#define FG_FORM_SLOT_LINE 5       /* y-line kernels (mode 1, and the array form of the Helmholtz solve) */
/* basis changes: MFMA GEMM split-K | 64 x 64 tile | 128 x 128 tile | 64 x 128 tile with the whole K (64-plane z transform) | row FFT
 * of the cosine basis | row FFT of the Fourier basis | the fp64 build's plain kernels */
#define FG_FORM_GEMM_SPLITK 1
#define FG_FORM_GEMM_T64 2
#define FG_FORM_GEMM_T128 3
#define FG_FORM_GEMM_Z64 4
#define FG_FORM_DCT 5
#define FG_FORM_FFT 6
#define FG_FORM_F64 7
/* tridiagonal solve: streaming | three LDS arrays | two LDS arrays | the same, making the row-mean factors (FAC) | fp64 kernel */
#define FG_FORM_TRI_STREAM 1
#define FG_FORM_TRI_LDS3 2
#define FG_FORM_TRI_LDS2 3
#define FG_FORM_TRI_LDS3_FAC 4
#define FG_FORM_TRI_LDS2_FAC 5
#define FG_FORM_TRI_F64 6
/* factors: the grid's A = 1 operator | per-env row-mean factors read from memory | made by the FAC launch itself */
#define FG_FORM_FAC_GRID 1
#define FG_FORM_FAC_ROWMEAN 2
#define FG_FORM_FAC_MADE 3
/* Helmholtz: array form (k_helm_coeffs + the y-line kernels) | row form with 32 | 64 columns per workgroup */
#define FG_FORM_HELM_ARRAY 1
#define FG_FORM_HELM_ROW32 2
#define FG_FORM_HELM_ROW64 3
/* y-line: column block in LDS | streaming */
#define FG_FORM_LINE_LDS 1
#define FG_FORM_LINE_STREAM 2
/* mode 3 of fg_set_advection_preconditioner: every advection-diffusion solve right-preconditioned by the separable Helmholtz
 * operator I/dt - nu Laplacian (the matrix without its advective part), inverted by fast diagonalisation: basis change along the
 * PERIODIC, uniform transform axes (x, z; the eigenvectors of fg_set_fd_preconditioner), one tridiagonal solve along y per mode
 * and env.  lam_host [nz][nx]: sum of the transform axes' eigenvalues per mode (fluidgym_amd/simulation/fd_precond.py).  No
 * reference counterpart (its preconditioner for these solves is ILU(0), off by default); fp32 library only. */
int fg_set_fd_helmholtz(fg_handle h, const float* lam_host);
int fg_advection_retries(fg_handle h, int64_t* out, int32_t reset);
/* The reference's retry ladder of a linear solve (_linear_solve_wrapper, pict/PISOtorch_diff.py:410-476) on the single-block path.
 * fg_set_double_fallback(on): `solver_double_fallback` -- a solve that failed in fp32 (advection-diffusion BiCGStab: not converged;
 * pressure CG, which runs with returnBestResult: non-finite) is repeated in fp64 on the same fp32 matrix and right-hand side from a
 * cleared result (csrMat.toType(dp), rhs.to(dp)), BEFORE the preconditioned rung of fg_set_advection_preconditioner (modes 2 / 5).
 * fg_ladder: out4 = how often each rung ran since fg_create {advection fp64, advection preconditioned, pressure fp64, 0};
 * force_mask >= 0 (tests) makes first attempts count as failed: 1 advection, 2 pressure, 4 also the advection fp64 rung; -1 = only read. */
int fg_set_double_fallback(fg_handle h, int on);
/* fg_set_advection_jacobi(on): the velocity systems of uniform 2-D grids with walls in y (the channel family) are solved by point-Jacobi
 * sweeps, several per pass over the field with the tile kept on chip (csrc/fg_jacobi.hip), instead of the reference's BiCGStab
 * (bicgstab_solver_kernel.cu, called from PISOtorch_simulation.py:1735-1742) -- same system, same criterion (RMS residual < tol), another
 * iteration; a solve the sweeps do not settle goes to BiCGStab from a cleared start vector.  Off until called (the Python Simulation
 * calls it, policy `advection_jacobi`); FG_ADV_JACOBI=0/1 in the environment overrides.  fg_advection_jacobi_counts: solves settled
 * by the sweeps, solves handed on to BiCGStab. */
int fg_set_advection_jacobi(fg_handle h, int on);
int fg_advection_jacobi_counts(fg_handle h, int64_t* out2);
int fg_ladder(fg_handle h, int64_t* out4, int32_t force_mask);
/* Which kernels the NEXT un-preconditioned advection-diffusion solve of `nc` right-hand sides will run (tests, bench reports):
 * 0 = five kernels per BiCGStab iteration, 1 = two brick kernels (csrc/fg_bicgstab.hip k_bicgf_a / _b), 2 = two z-marching
 * LDS-ring kernels (csrc/fg_bicgstab3d.hip: 3-D grids that fit the tiles and fill the chip).  Replaces nothing in the reference
 * (bicgstab_solver_kernel.cu:63-411 has one form). */
int fg_advection_solver_form(fg_handle h, int nc, int32_t* out);
/* CopyScalarResultToBlocks (:6558-6746) */
int fg_copy_scalar_result_to_blocks(fg_handle h, int channel, void* stream);
/* SetupPressureMatrix (:5599-5615, kernel :4812-4978): rA = 1/A */
int fg_setup_pressure_matrix(fg_handle h, void* stream);
/* SetupPressureRHS (:5655-5672, kernels :5136-5255 + :5389-5434): h = H(u~), b = div h */
int fg_setup_pressure_rhs(fg_handle h, const fg_real* dt_B, void* stream);
/* SolveLinear(P, div, x, useBiCG=False) + `p -= mean(p)` (PISOtorch_simulation.py:1804-1821) +
 * CopyPressureResultToBlocks.  method = FG_SOLVER_*.  info_host: B entries. */
int fg_solve_pressure(fg_handle h, int method, fg_real tol, int max_iterations, int use_previous,
                      fg_solve_info* info_host, void* stream);
/* Opt-in accuracy mode of the pressure solves of this handle (round 6): mixed-precision iterative refinement -- the iterate is kept
 * in fp64, r = b - P x is formed in fp64 with the fp32 matrix entries promoted (what the reference's fp64 fallback does with its CSR
 * values, PISOtorch_diff.py:418-445), each correction P d = r / |r| is solved by the fp32 solver to `inner_relative_tol`, at most
 * `max_corrections` times or until RMS(r) < target_tol.  0 corrections = off (default).  fp32 library only. */
int fg_set_pressure_refinement(fg_handle h, int32_t max_corrections, fg_real target_tol, fg_real inner_relative_tol);
/* CorrectVelocity(version=1) (:6220-6236, kernel :5962-5995 + :816-849) */
int fg_correct_velocity(fg_handle h, void* stream);
/* CopyVelocityResultToBlocks / FromBlocks (:6558-6746) */
int fg_copy_velocity_result_to_blocks(fg_handle h, void* stream);
int fg_copy_velocity_result_from_blocks(fg_handle h, void* stream);

/* ---- fused driver: one _PISO_split_step without Python hooks --------------------------------
 * (PISOtorch_simulation.py:1431-2002, orthogonal branch).  buoyancy_axis >= 0 fuses the RBC
 * PRE_VELOCITY_SETUP hook: velocitySource[axis] = buoyancy_factor * T (rbc_env_base.py:285-297).
 * stats_host (optional, 4 ints): max iterations of {scalar, velocity, pressure0, pressure1}. */
typedef struct fg_step_options {
    int32_t corrector_steps;      /* 2 */
    int32_t advect_scalar;        /* solve passive scalars first */
    int32_t pressure_method;      /* FG_SOLVER_* */
    int32_t max_iterations;       /* 5000 (PISOtorch_simulation.py:564) */
    fg_real advection_tol;          /* RMS residual, 1e-5 default (PISOtorch_diff.py:247-253) */
    fg_real pressure_tol;
    int32_t buoyancy_axis;        /* -1 = none */
    fg_real buoyancy_factor;
    int32_t pressure_warm_start;  /* 1: start each pressure solve from the previous pressureResult (the
                                     reference passes x=None in its orthogonal branch and pressureResult
                                     in its non-orthogonal branch, PISOtorch_simulation.py:1804-1812 vs
                                     :1878-1882; the converged answer is the same) */
} fg_step_options;
int fg_piso_step(fg_handle h, const fg_real* dt_B, const fg_step_options* opt, int32_t* stats_host,
                 void* stream);
/* Iteration statistics of the linear solves since the last reset (host bookkeeping of the LinearSolverResultInfo every
 * SolveLinear call returns, bicgstab_solver.h): out13 = sum of iterations [4] | systems solved [4] | max iterations [4] |
 * PISO steps, kinds = {passive scalar, velocity, pressure corrector 0, pressure corrector 1}; a system = env x component.
 * reset != 0 clears them after the read. */
int fg_solver_counters(fg_handle h, int64_t* out13_host, int32_t reset);
/* per kind, the systems whose solve ended WITHOUT meeting its tolerance since the last reset of the counters (iteration cap
 * reached, best iterate returned: LinearSolverResultInfo.converged == false); cleared together with fg_solver_counters */
int fg_solver_unconverged(fg_handle h, int64_t* out4_host);
/* Simulation.single_step entirely on the native side (simulation.py:206-280 + _PISO_adaptive_step,
 * PISOtorch_simulation.py:2004-2064): flux-balance guard, per-env adaptive substeps
 * ts = t_rem / ceil(t_rem / (CFL / max_vel)) recomputed before every substep, the advective-outflow PRE
 * hook (update_advective_boundaries + balance_boundary_fluxes, :228-393) and fg_piso_step per substep.
 * One device->host read per substep (flux balance + max velocity), as in the reference, but no
 * interpreter in the loop.  out_host: [0..3] max solver iterations {scalar, velocity, pressure0,
 * pressure1} of the last substep, [4] substeps taken, [5] 1 if every solve converged;
 * flux_balance_host (optional, B floats) receives the guard values. */
typedef struct fg_sim_options {
    fg_step_options step;
    fg_real time_step;          /* physical time advanced per call */
    fg_real cfl;                /* adaptive_CFL */
    int32_t adaptive;         /* 1: substeps == -1 ("ADAPTIVE"); 0: `substeps` fixed steps of time_step */
    int32_t substeps;
    fg_real flux_balance_tol;   /* 1e-5 */
    int32_t outflow_mask;     /* bit f: FIXED face f is an advective outflow (0 = none) */
    fg_real outflow_velm[3];    /* characteristic velocity u_m */
    fg_real outflow_tol;        /* flux re-balancing triggers above 0.01 * outflow_tol */
    int32_t max_substeps;     /* safety cap (reference warns above 1000) */
} fg_sim_options;
int fg_single_step(fg_handle h, const fg_sim_options* opt, int32_t* out_host_6, fg_real* flux_balance_host,
                   void* stream);
/* fg_multi_step: `n` calls of fg_single_step in one C call -- the sim steps of one env step (FluidEnv.step runs
 * int(step_length / dt) of them, fluid_env.py:840-842) without a return to the interpreter in between.  bvel_schedule (optional,
 * n x 6 pointers, step-major): boundary velocity tensor bound to face f before sim step k, NULL = keep what is bound (the
 * smoothed control of the jets changes every sim step, cylinder_env_base.py:748-753).  out_host_6n receives the six words of
 * every step; steps_done the number of steps completed (n unless a step returned an error, which is passed on). */
int fg_multi_step(fg_handle h, const fg_sim_options* opt, int32_t n, const fg_real* const* bvel_schedule, int32_t* out_host_6n,
                  fg_real* flux_balance_host, int32_t* steps_done, void* stream);
/* make_divergence_free (PISOtorch_simulation.py:1320-1429) */
int fg_make_divergence_free(fg_handle h, fg_real tol, int max_iterations, fg_solve_info* info_host,
                            void* stream);

/* ---- access to solver vectors (tests / fixtures) -------------------------------------------- */
enum fg_buffer {
    FG_BUF_A = 0,          /* Adiag [B,N]                               */
    FG_BUF_C_OFF = 1,      /* C off-diagonals [B,2d,N] (face order)     */
    FG_BUF_ADV_RHS = 2,    /* velocityRHS [B,d,N] / scalarRHS [B,N]     */
    FG_BUF_VEL_RESULT = 3, /* velocityResult [B,d,N]                    */
    FG_BUF_H = 4,          /* pressureRHS (h) [B,d,N]                   */
    FG_BUF_DIV = 5,        /* pressureRHSdiv [B,N]                      */
    FG_BUF_P_RESULT = 6,   /* pressureResult [B,N]                      */
    FG_BUF_SCALAR_RESULT = 7 /* scalarResult [B,N] (one channel)        */
};
/* velocityResult := block velocity, pressureResult := 0 (call after re-initialising the fields) */
int fg_reset_solver_state(fg_handle h, void* stream);
/* The single-block handle's counterpart of fg_mb_solver_hints: per solve kind (4) the sweeps the last Jacobi solve needed, the
 * solves still to skip after a failure, the failures in a row (csrc/fg_jacobi.hip) -- 12 words that decide which iteration runs.
 * Domain.Clone / Restore carry them (reference: envs/fluid_env.py:1320-1363); fg_reset_solver_state clears them.  set = 0 reads. */
int fg_solver_hints(fg_handle h, int32_t* hints12, int32_t set);

/* ---- per-env restore from a bank of stored states (csrc/fg_envrestore.hip) ---------------------
 * One record per env to restore: env `env` of the batch becomes state `src` of the bank, mirrored (flip) and then rolled (shift)
 * along the periodic axes -- torch.roll(torch.flip(t, [-1]), shift_x, -1) and the same along z -- with the sign change of the
 * mirrored velocity component (rbc_env_base.py:335-362). */
typedef struct fg_env_sel {
    int32_t env, src;          /* destination env in [0, B), source state in [0, S)        */
    int32_t flip_x, flip_z;    /* 0 / 1                                                     */
    int32_t shift_x, shift_z;  /* in [0, nx) / [0, nz)                                      */
} fg_env_sel;
/* dst[env, c, z, y, x] = sign(c) * bank[src, c, zs, y, xs] for every record, xs = flip_x ? nx-1 - ((x - shift_x) mod nx) :
 * (x - shift_x) mod nx, zs likewise; dst is the bound field `which_field` (an fg_field id: FG_VELOCITY, FG_PRESSURE, FG_SCALAR,
 * FG_VELOCITY_SOURCE, FG_BOUND_VELOCITY + face, FG_BOUND_SCALAR + face) and bank [S, C, ...] a device array of S states of that
 * field's per-env layout.  signed_components (0 / 1; vector fields only): component 0 changes sign under flip_x, component 2 under
 * flip_z.  A face array has extent 1 along its normal axis, which is a FIXED axis and carries no transform.  Envs not named in sel
 * are not written.  sel is a HOST array (it is checked here, then uploaded to an array the handle owns and read by the one launch);
 * the call is asynchronous on `stream`, every value is a copy or a negation (bit-exact).
 * FG_ERR_INVALID_ARG before any launch: a null pointer, S < 1, n_sel outside 1..B, an env or src out of range, an env named twice,
 * a flip that is not 0 / 1, a shift outside [0, n), a flip or shift along an axis with FIXED faces, flip_z or shift_z on a 2-D grid,
 * signed_components on a field that is not a vector field, an unknown field id; FG_ERR_NOT_BOUND: the field is not bound. */
int fg_env_restore_field(fg_handle h, int which_field, const fg_real* bank, int32_t S, const fg_env_sel* sel, int32_t n_sel,
                         int32_t signed_components, void* stream);
/* fg_reset_solver_state for the envs named in sel (only `env` of each record is read): their slice of pressureResult := 0, of
 * velocityResult := block velocity.  The host-side hints of fg_solver_hints belong to the handle, not to an env, and stay. */
int fg_env_reset_solver_state(fg_handle h, const fg_env_sel* sel, int32_t n_sel, void* stream);
int fg_get_buffer(fg_handle h, int which, fg_real** out_ptr, int64_t* out_count);
/* device-to-device copy of a solver vector into a caller buffer of fg_get_buffer's count */
int fg_read_buffer(fg_handle h, int which, fg_real* dst, void* stream);

/* ---- standalone pressure-Poisson kernels on caller arrays (micro-benchmark / tests) ----------
 * Operator: (P x)_c = sum_f off_f (x_N - x_c), off_f = (alpha_P rA_P + alpha_N rA_N)/2, no entry at
 * FIXED faces (PISO_multiblock_cuda_kernel.cu:4842-4889).  All arrays [B,N]. */
int fg_poisson_apply(fg_handle h, const fg_real* rA, const fg_real* x, fg_real* y, void* stream);
/* n_sweeps damped-Jacobi / red-black Gauss-Seidel sweeps on P x = b (x updated in place; Jacobi
 * uses the handle's scratch vector).  omega = relaxation factor. */
int fg_poisson_jacobi(fg_handle h, const fg_real* rA, const fg_real* b, fg_real* x, int n_sweeps, fg_real omega,
                      void* stream);
int fg_poisson_rbgs(fg_handle h, const fg_real* rA, const fg_real* b, fg_real* x, int n_sweeps, fg_real omega,
                    void* stream);
/* n_iterations of CG without convergence polling (timing) -- or a full solve when tol > 0. */
int fg_poisson_cg(fg_handle h, const fg_real* rA, const fg_real* b, fg_real* x, fg_real tol, int max_iterations,
                  int use_x0, fg_solve_info* info_host, void* stream);
/* same with the fast-diagonalisation preconditioner (FG_SOLVER_FDCG) */
int fg_poisson_fdcg(fg_handle h, const fg_real* rA, const fg_real* b, fg_real* x, fg_real tol, int max_iterations,
                    int use_x0, fg_solve_info* info_host, void* stream);

/* ---- live kernel timing for bench.py's roofline -----------------------------------------------
 * When enabled, every FG_PROF_PERIOD-th launch (default 32) of each solver kernel kind is issued with a
 * start/stop event pair on the solve's stream (kernel-accurate timestamps), and the systems still
 * iterating in that launch are counted on the device.  Kinds are 0 .. fg_profile_kinds()-1, named by
 * fg_profile_kind_name (k_cg_ap, k_cg_update, k_bicg_p/v/s/t/x, k_gemm_f32, k_gemm_sk, k_tridiag_y).
 * fg_profile_read returns for one kind: summed milliseconds and count of the sampled launches that did
 * work, their summed ALGORITHMIC bytes and flops (active systems x per-system figure),
 * the same restricted to launches in which every system was active, and the total launches of that kind
 * (sampled or not) since fg_profile_enable, and milliseconds / count over ALL sampled launches including
 * those that found every system converged (the figure rocprofv3 --stats averages).  Any output pointer
 * may be NULL.  Synchronises the device. */
/* STREAM triad a = b + scalar * c over n floats (n % 4 == 0), `reps` launches timed with events on `stream`: the measured
 * practical HBM roof beside the spec figure (bytes per launch = 12 n).  Synchronises. */
int fg_stream_triad(float* a, const float* b, const float* c, float scalar, int64_t n, int32_t reps, float* ms_per_launch, void* stream);
/* Litmus for the access pattern of the multi-kernel Krylov recurrences: `iterations` x five launches over
 * `nsys` systems of `cells` cells; sums accumulated with device-scope atomics are read by the following kernel and zeroed by a
 * leader workgroup; atomic_access = 10 x store + load with load 0 plain / 1 agent-scope atomic load and store 0 plain / 1
 * agent-scope atomic store / 2 atomic exchange (0 = the round-1 pattern).  bad_reads[12] counts, per slot of the record, reads that did not return the full sum
 * ([11]: reads of a flag word stored by the leader one to four kernels earlier that did not return it), bad_value[12] keeps the
 * first wrong value.  Synchronises. */
int fg_coherence_litmus(int32_t atomic_access, int32_t nsys, int32_t cells, int32_t iterations, int64_t* bad_reads, double* bad_value,
                        void* stream);
/* Order-independent reduction accumulator of the Krylov solvers (csrc/fg_internal.h FgDacc: every contribution split exactly into
 * four 42-bit fixed-point words added with integer atomics, so a dot product does not depend on the arrival order of the
 * workgroups -- what the reference gets from cuBLAS dots in a fixed order, cg_solver_kernel.cu:277,317).  fg_dacc_host_sum
 * evaluates plain + sum(values) with the very split / read-back code the kernels run (no GPU needed); fg_dacc_device_sum does the
 * same sum `reps` times on the device, one atomic contribution per thread with a different launch shape each time.  A value
 * that is NaN, Inf or >= 2^75 in magnitude makes the sum NaN. */
int fg_dacc_host_sum(const double* values, int64_t n, double plain, double* out_sum);
int fg_dacc_device_sum(const double* values_host, int64_t n, double plain, int32_t reps, double* out_sums_host, void* stream);
/* ---- field summaries for the domain statistics (csrc/fg_fieldstats.hip; both libraries, handle-free) ---------------------
 * One sample of FluidEnv.compute_domain_statistics: per-env moments and a per-env histogram of a contiguous device field
 * [batch, channels, n] of fg_real (single-block [B,d,(Z,)Y,X], pressure [B,1,...], the multi-block flat [B,d,N]).  The value of a
 * cell is component `channel`, or with channel = -1 the Euclidean magnitude over all channels (squares accumulated in fp64 in
 * ascending channel order, then sqrt).  Two jobs, either or both in the one launch over the field:
 *   moments    (workspace, moments, counts all non-NULL; all NULL = skipped)  moments[batch][3] = min, max over the finite cells
 *              and their sum through the exact accumulator above (bit-equal to fg_dacc_host_sum over the same values; exact for
 *              up to 2^20 cells per env and |value| < 2^75, as there); counts[batch][2] = finite cells, non-finite cells.  An env
 *              without a finite cell reports NaN, NaN, 0.  workspace: batch * FG_FIELD_SUMMARY_WORK_BYTES device bytes, 64-byte
 *              aligned, initialised and consumed by the call.
 *   histogram  (hist non-NULL)  hist[batch][nbins] 64-bit counts, nbins in 1..4096, width > 0: the call ADDS one to bin
 *              clamp(floor((double(v) - lo) / width), 0, nbins - 1) for every finite cell (fp64 IEEE subtraction and division: the
 *              host expression gives the same bin); the caller zeroes the array.  Non-finite cells are not binned.
 * Every cross-workgroup combination is an integer atomic (order-preserving keys for min / max, fixed-point words for the sum), so
 * an env's outputs depend neither on the launch order nor on the rest of the batch.  All outputs are device arrays; the call is
 * asynchronous on `stream`.  FG_ERR_INVALID_ARG: a null pointer, n <= 0, batch outside 1..65535, channel outside -1..channels-1,
 * nbins outside 1..4096 or width <= 0 with a histogram. */
#define FG_FIELD_SUMMARY_WORK_BYTES 128
int fg_field_summary(const fg_real* field, int32_t batch, int32_t channels, int64_t n, int32_t channel, void* workspace,
                     double* moments, int64_t* counts, double lo, double width, int32_t nbins, uint64_t* hist, void* stream);
/* ---- online plane-averaged flow statistics (csrc/fg_planestats.hip; both libraries, handle-free) ------------------------------
 * One sample of PlaneMoments (simulation/plane_stats.py; the reference's WelfordOnlineParallel_Torch, CovarianceOnlineParallel_Torch
 * and MultivariateMomentsOnlineParallel_Torch, online_statistics.py:31-266, 419-787): for every row (env, y) the mean over (z, x) of K
 * channels and the sums of products of their deviations from that mean, merged into running accumulators on the device in ONE launch.
 *   channels[k]      HOST table of K device pointers: cell (env, z, y, x) of channel k is
 *                    channels[k][env * batch_stride[k] + (z * ny + y) * nx + x]; batch_stride (HOST table, in reals, each >= nz * ny * nx)
 *                    lets a caller pass the component slices of velocity [B, d, (Z,) Y, X], pressure [B, 1, ...] and passiveScalar in
 *                    place.  Both tables are copied into the kernel arguments: no device table, no host-to-device copy.  2-D: nz = 1.
 *   K                3..5 (u,v,p / u,v,w,p or u,v,p,T / u,v,w,p,T: the kernel does not care what a channel means)
 *   order            2..4
 *   n [batch], mean [batch][ny][K], central [batch][ny][M]: fp64 device accumulators, updated in place.  central holds, in this order,
 *                    the K (K + 1) / 2 sums of d_i d_j for i <= j (i ascending, then j), for order >= 3 the K sums of d_i^3, for order 4
 *                    the K sums of d_i^4.  The sample's mean and central sums are taken in fp64 (two passes over the plane) and merged
 *                    by the pairwise update of Pebay et al. 2016 with delta = mean_sample - mean_running; an env with n = 0 stores the
 *                    sample.  n advances by nz * nx per call.
 *   tickets [batch]  64-bit device counters that order the one write of n[env] after the reads of it by the env's rows.  The caller
 *                    zeroes n and tickets together before the first sample (mean and central need no initialisation) and keeps ny.
 * One workgroup (one wave for planes of up to 1024 cells) owns a row and reduces in a fixed tree: no floating-point atomics, so a row's
 * result depends neither on the launch order nor on the other envs nor on `batch`, and repeats bit for bit.  16-byte loads are used
 * when nx and every batch stride are multiples of 16 bytes / sizeof(fg_real) and every channel pointer is 16-byte aligned, scalar loads
 * otherwise.  A non-finite cell makes the sample, hence the accumulators, of its row NaN (all channels) and nothing else.  Asynchronous
 * on `stream`; nothing returns to the host.  FG_ERR_INVALID_ARG: a null pointer, K outside 3..5, order outside 2..4, a non-positive
 * extent, a batch stride below nz * ny * nx, nz * nx above 2^30 or batch * ny above 2^31 - 1. */
int fg_plane_moments(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz, int32_t ny,
                     int32_t nx, int32_t order, double* n, double* mean, double* central, uint64_t* tickets, void* stream);
/* ---- online temporal two-point correlations of wall-parallel planes (csrc/fg_planetimecorr.hip; both libraries, handle-free) ------
 * One sample of PlaneTimeCorrelation (simulation/plane_timecorr.py; the reference's TemporalTwoPointCorrelation_Online_torch,
 * online_statistics.py:1271-1343): for every row (env, y) and channel k the fluctuation c' = c - mean_{z,x}(c) of the plane is
 * correlated with the fluctuations b' the same plane had at earlier samples, kept in a ring of base slots, in ONE launch.
 *   channels[k], batch_stride[k]   HOST tables of K = 1..5 entries, addressed as for fg_plane_moments (fields read in place, both
 *                    tables copied into the kernel arguments).
 *   lags             lags recorded, 0 .. lags - 1 samples.
 *   slot_lag [n_slots]   HOST table, n_slots = 1..8, read during the call: what each slot does at this sample.  -1: idle.  0: this
 *                    sample's c', rounded to fg_real, is stored as the slot's base and correlated with itself -- the slot's sum of
 *                    b'^2 and its cross term are taken from the stored (rounded) values, so lag 0 and the later lags see one base.
 *                    l > 0: the sample is correlated with the stored base, at lag l.  Two slots never hold the same lag >= 0.
 *   base [n_slots][batch][K][nz][ny][nx]   DEVICE, fg_real: the stored fluctuations.
 *   base_ss [n_slots][batch][ny][K]        DEVICE, fp64: the sum of b'^2 over the plane, written with the base.
 *   acc [batch][ny][K][lags][4]            DEVICE, fp64, zeroed by the caller before the first sample.  For every live slot, at its
 *                    lag l, four values are ADDED: the coefficient sum b'c' / sqrt(sum b'^2 sum c'^2), sum b'c' / cells,
 *                    sum b'^2 / cells and sum c'^2 / cells (cells = nz nx).  How many bases have reached a lag is the caller's
 *                    count: the schedule is the caller's, so two records merge by addition.
 * Two fp64 passes per channel of a row: the plane sum for the mean, then the same cells again for the sums.  Ownership and order are
 * those of fg_plane_moments (one workgroup, or one wave for planes of up to 1024 cells, per row; fixed tree; no floating-point
 * atomics; every accumulator element and every base cell written by exactly one thread): a row's result depends only on its cells,
 * its stored bases and the extents, and repeats bit for bit.  16-byte loads and stores when nx and every batch stride are multiples of
 * 16 bytes / sizeof(fg_real) and every channel pointer and base are 16-byte aligned, scalar ones otherwise.  Nothing is filtered: a
 * non-finite cell makes all four entries of its row and channel NaN at the lags this sample touches -- at every lag of the base when
 * the sample is stored as one -- and nothing else.  A plane of one cell has no fluctuation: coefficient 0 / 0 = NaN, the sums 0.
 * Asynchronous on `stream`; nothing returns to the host; a sample whose slots are all idle launches nothing.  FG_ERR_INVALID_ARG: a
 * null pointer, K outside 1..5, lags < 1, n_slots outside 1..8, a slot_lag entry outside [-1, lags), two slots with the same
 * lag >= 0, a non-positive extent, a batch stride below nz * ny * nx, nz * nx above 2^30 or batch * ny above 2^31 - 1. */
int fg_plane_timecorr(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz, int32_t ny,
                      int32_t nx, int32_t lags, int32_t n_slots, const int32_t* slot_lag, fg_real* base, double* base_ss, double* acc,
                      void* stream);
/* ---- online Welch power and cross spectra of per-env signals (csrc/fg_signalspectra.hip; both libraries, handle-free) ------------
 * One sample of SignalSpectra (simulation/signal_spectra.py) for a batch of envs in ONE launch; nothing returns to the host and the
 * host decides nothing per env.
 *   sources[i], batch_stride[i], widths[i]   HOST tables of n_sources = 1..8 entries, copied into the kernel arguments: source i is a
 *                    DEVICE array of fg_real read in place, value c < widths[i] of env b at sources[i][b * batch_stride[i] + c].  The
 *                    signals are the columns of the sources one after the other, S = sum widths = 1..64.
 *   segment, noverlap   L, a power of two from 16 up to 4096 (fp32) / 2048 (fp64), and 0 <= noverlap < L; hop = L - noverlap.
 *   detrend          per segment and signal: 0 none, 1 the mean, 2 the least-squares line (sums in fp64).
 *   window [L]       DEVICE, fp64: made by the caller, so any window works.
 *   pairs [n_pairs][2]   HOST table of n_pairs = 0..64 signal pairs (a, b), copied into the kernel arguments.
 *   ring [batch][S][L]   DEVICE, fg_real: the last L samples of every signal; the sample lands at fill[b] % L.
 *   fill [batch]     DEVICE, int64: samples since the env last (re)started, incremented here.  The caller zeroes the entries of the
 *                    envs it restarts: their open segment is dropped, the accumulators stay.
 *   power [batch][S][L/2+1], cross [batch][n_pairs][L/2+1][2], segments [batch] (int64)   DEVICE, zeroed by the caller before the first
 *                    sample.  For every env with fill >= L and (fill - L) % hop == 0 after the append, the L ring values of each
 *                    signal in time order are detrended, multiplied by the window, rounded to fg_real and transformed (a Stockham
 *                    FFT in LDS); |X_s|^2 is ADDED to power, conj(X_a) X_b (re, im) to cross, 1 to segments, all evaluated in fp64
 *                    with DC and Nyquist kept.  cross may be null when n_pairs is 0.
 *   last [batch][S][L/2+1]   DEVICE or null: overwritten with |X_s|^2 of the segment just processed.
 * One workgroup per env; every signal is transformed on its own, so its numbers are a function of its own L samples, the window and
 * the detrend and of nothing else: not of batch, of the env's row, of the other signals or of which other envs had a segment due.  Every
 * accumulator element has one writer; no floating-point atomics.  A non-finite value among the L samples of a signal makes that
 * signal's power (from then on) and `last`, and the cross spectra of its pairs, NaN, and changes nothing else.  Asynchronous on
 * `stream`.  FG_ERR_INVALID_ARG: a null pointer (cross and pairs only with n_pairs > 0; last may be null), n_sources outside 1..8, a
 * width below 1 or S above 64, a batch stride below its width, n_pairs outside 0..64, a pair index outside [0, S), a non-positive
 * batch, noverlap outside [0, segment), detrend outside 0..2.  FG_ERR_UNSUPPORTED: a segment that is no power of two, below 16, or
 * whose twiddles and three work buffers of `segment` complex fg_real exceed 160 KB of LDS. */
int fg_signal_spectra(const fg_real* const* sources, const int64_t* batch_stride, const int32_t* widths, int32_t n_sources, int32_t batch,
                      int32_t segment, int32_t noverlap, int32_t detrend, const double* window, const int32_t* pairs, int32_t n_pairs,
                      fg_real* ring, int64_t* fill, double* power, double* cross, int64_t* segments, double* last, void* stream);
/* ---- online per-cell flow statistics of multi-block domains (csrc/fg_cellstats.hip; both libraries, handle-free) ----------------
 * One sample of CellMoments (simulation/cell_moments.py; the reference's WelfordOnlineParallel_Torch and
 * CovarianceOnlineParallel_Torch applied per block with dims = [0] in 2-D and [0, 2] in 3-D, online_statistics.py:31-266): for every
 * column of every env the mean of the K = dims + 1 channels u, v(, w), p over the column's nz cells and the K (K + 1) / 2 sums of
 * products of deviations from it, merged into running accumulators on the device in ONE launch.
 *   velocity [batch][dims][n_cells], pressure [batch][n_cells]   the flat fields of a multi-block domain, contiguous, read in place
 *   block_table      HOST table of n_blocks (1..8) rows (cell_offset, layer_cells, nz, column_offset), copied into the kernel
 *                    arguments: cell z of column c (0 <= c < layer_cells) of a block is field[cell_offset + z * layer_cells + c], its
 *                    accumulators are column column_offset + c.  2-D, or no span averaging: nz = 1 and layer_cells = the block's
 *                    cells.  nz may differ from block to block.  column_offset must be the sum of layer_cells of the rows before; NC
 *                    is the sum over all rows.
 *   samples          calls already merged into the accumulators, counted by the HOST: a column has seen n_A = samples * nz cells.
 *                    0 stores the sample (mean and central need no initialisation).  The device keeps no counter.
 *   mean [batch][K][NC], central [batch][K (K + 1) / 2][NC]   fp64 device accumulators, updated in place; central holds the sums of
 *                    d_i d_j for i <= j (i ascending, then j).  The sample's mean and central sums are taken in fp64, the cells in
 *                    ascending z, and merged by the order-2 rule of fg_plane_moments with n_B = nz.
 * A thread owns a column (16-byte loads: 16 / sizeof(fg_real) neighbouring columns, each with sums of its own); no floating-point
 * atomic, no cross-lane operation, and the file is compiled with -ffp-contract=off (every product and sum rounded on its own): a
 * column's result depends on its own cells and `samples` only -- not on `batch`, the other envs or blocks, the load form or the
 * launch order -- and repeats bit for bit.  16-byte loads are used in a block whose
 * cell_offset, layer_cells and column_offset are multiples of 16 / sizeof(fg_real) when n_cells and NC are too and all four pointers
 * are 16-byte aligned; scalar loads otherwise.  A non-finite cell makes the accumulators of its column NaN (all channels) and nothing
 * else.  Asynchronous on `stream`; nothing returns to the host.  FG_ERR_INVALID_ARG: a null pointer, dims outside 2..3, batch outside
 * 1..65535, n_cells outside 1..2^31 - 1, n_blocks outside 1..8, samples outside 0..2^40 - 1, a non-positive layer_cells or nz, cells
 * of a block outside the field, a column_offset that is not the running sum. */
int fg_mb_cell_moments(const fg_real* velocity, const fg_real* pressure, int32_t dims, int32_t batch, int64_t n_cells,
                       const int64_t* block_table, int32_t n_blocks, int64_t samples, double* mean, double* central, void* stream);
/* What a thread of that launch would own in every block: widths[i] = 1 (one column, scalar loads) or 16 / sizeof(fg_real) (that many
 * neighbouring columns, 16-byte loads), decided by the same code from the same pointers and table.  Host only: nothing is
 * dereferenced but block_table and widths, nothing is launched.  Same argument checks and codes as fg_mb_cell_moments. */
int fg_mb_cell_moments_widths(const fg_real* velocity, const fg_real* pressure, int64_t n_cells, const int64_t* block_table,
                              int32_t n_blocks, const double* mean, const double* central, int32_t* widths);
/* ---- wall distributions of multi-block domains and their online statistics (csrc/fg_wallstats.hip; both libraries, handle-free) --
 * The integrand of fg_mb_wall_forces per wall face (WallRing.distribution, envs/forces.py) and one sample of WallMoments
 * (simulation/wall_stats.py): the reference sums the traction over the ring (compute_forces_2d / _3d, envs/util/forces.py:193-377)
 * and keeps no curve.
 *   velocity [batch][dims][n_cells], boundary_velocity [batch][dims][n_slots], pressure [batch][n_cells]
 *                    the flat fields of a multi-block domain, contiguous, read in place (the in-plane components 0 and 1 are read)
 *   cell_index, slot_index [layers][n]   int32, DEVICE: wall-adjacent cell and boundary slot of every face, in ring order
 *   geom [5][n]      DEVICE: normal x, normal y, tangential spacing, wall distance, face length (the packing of fg_mb_wall_forces;
 *                    the face length is not read)
 *   viscosity, viscosity_B   the scalar, or (non-NULL) one viscosity per env, [batch] on the device
 * A face (b, layer, j) is the arithmetic of fg_mb_wall_forces without the face length -- neighbours cl = ci[j + 1 mod n],
 * cr = ci[j - 1 mod n], dn = (u[c] - ub[slot]) / distance, dt = (u[cr] - u[cl]) / (2 spacing), the composed gradients, sxy -- and
 * gives four channels in fg_real:
 *   0  p      the pressure of the wall-adjacent cell
 *   1  tau_w  the viscous traction along the ring tangent t = (ny, -nx)
 *   2  fx     (2 nu du_dx - p) nx + 2 nu sxy ny
 *   3  fy     2 nu sxy nx + (2 nu dv_dy - p) ny
 * The file is compiled with -ffp-contract=off: every product, sum and division is rounded on its own, a face depends on its own
 * cells only -- not on `batch`, the other envs or the launch -- and repeats bit for bit; both entries compute the same bits.  An
 * index outside [0, n_cells) / [0, n_slots) is not dereferenced: its face is NaN in all four channels.
 * fg_mb_wall_distribution: out [batch][4][layers][n], one thread per face, ONE launch.
 * fg_mb_wall_moments: a record is face j over all layers (span_average != 0: R = n, n_B = layers) or one face (R = layers * n,
 * n_B = 1); per record the mean of the four channels over its faces and the 10 sums of d_i d_j (i <= j; i ascending, then j), both in
 * fp64, the layers ascending, in two passes, merged into mean [batch][4][R], central [batch][10][R] (fp64, device, updated in
 * place) by the order-2 rule of fg_plane_moments with n_A = samples * n_B.  `samples`: calls already merged, counted by the HOST; 0
 * stores the sample (the accumulators need no initialisation).  One thread per record, ONE launch; no floating-point atomic, no
 * cross-lane operation, no device counter.
 * Both are asynchronous on `stream`; nothing returns to the host.  FG_ERR_INVALID_ARG, before anything is launched: a null pointer
 * (viscosity_B excepted), dims outside 2..3, batch outside 1..65535, a non-positive n or layers, n_cells or n_slots outside
 * 1..2^31 - 1, more than 2^31 - 1 faces, samples outside 0..2^40 - 1. */
int fg_mb_wall_distribution(const fg_real* velocity, const fg_real* boundary_velocity, const fg_real* pressure, int32_t dims,
                            int32_t batch, int64_t n_cells, int64_t n_slots, const int32_t* cell_index, const int32_t* slot_index,
                            const fg_real* geom, int32_t n, int32_t layers, fg_real viscosity, const fg_real* viscosity_B, fg_real* out,
                            void* stream);
int fg_mb_wall_moments(const fg_real* velocity, const fg_real* boundary_velocity, const fg_real* pressure, int32_t dims, int32_t batch,
                       int64_t n_cells, int64_t n_slots, const int32_t* cell_index, const int32_t* slot_index, const fg_real* geom,
                       int32_t n, int32_t layers, fg_real viscosity, const fg_real* viscosity_B, int32_t span_average, int64_t samples,
                       double* mean, double* central, void* stream);
/* ---- online Reynolds-stress budgets of channel flows (csrc/fg_planebudgets.hip; both libraries, handle-free) -------------------
 * One sample of PlaneBudgets (simulation/plane_budgets.py; the reference's TurbulentEnergyBudgetsOnlineParallel_Torch,
 * online_statistics.py:790-1268): for every row (env, y) the means over (z, x) of K channels -- u, v, w, the three pressure gradients,
 * the nine velocity gradients, with forcing the three source components -- and the M sums of products of their deviations that the
 * budget terms need, merged into running accumulators on the device in ONE launch; the gradients are formed in registers.
 *   fields[f]        HOST table of n_fields device pointers in the order u, v, w, p (n_fields = 4: K = 15, M = 43) or
 *                    u, v, w, p, s_x, s_y, s_z (n_fields = 7: K = 18, M = 52); cell (env, z, y, x) of field f is
 *                    fields[f][env * batch_stride[f] + (z * ny + y) * nx + x], as for fg_plane_moments: the component slices of
 *                    velocity [B, 3, Z, Y, X], pressure [B, 1, Z, Y, X] and velocitySource are read in place.  Both tables are copied
 *                    into the kernel arguments.
 *   x [nx], y [ny], z [nz]   fp64 DEVICE arrays of cell-centre coordinates (strictly monotonic).  The gradient along an axis is
 *                    (f[i + 1] - f[i - 1]) / |pos[i + 1] - pos[i - 1]|; beyond an end the ghost position is mirrored (2 pos[0] - pos[1],
 *                    2 pos[n - 1] - pos[n - 2]) and the ghost value is 0 (the reference's _data_grad(borders="ZERO"), on y the wall).
 *   wrap_x, wrap_z   non-zero: the ghost VALUE on that axis is the cell at the other end (a periodic axis); the ghost distance stays the
 *                    mirrored one, exact on a uniform axis.  Zero: the reference's zero padding.
 *   n [batch], mean [batch][ny][K], central [batch][ny][M]: fp64 device accumulators, updated in place.  Channels: 0..2 u, v, w;
 *                    3..5 dp/dx, dp/dy, dp/dz; 6 + 3 k + i = d u_i / d x_k; 15..17 s_x, s_y, s_z.  central holds, in this order, the 6 sums
 *                    d_i d_j of (u, v, w) (i <= j), the 10 sums d_i d_j d_k (i <= j <= k), the 9 sums u_i' (dp/dx_j)' (i, then j), with
 *                    forcing the 9 sums u_i' s_j', then for k = 0..2 the 6 second-order sums of (d_k u, d_k v, d_k w).  Two fp64 passes
 *                    per sample and the pairwise update of Pebay et al. 2016 with delta = mean_sample - mean_running, mixed third-order
 *                    sums included; an env with n = 0 stores the sample.  n advances by nz * nx per call.
 *   tickets [batch]  as for fg_plane_moments: zeroed with n before the first sample.
 * Ownership and order are those of fg_plane_moments (one workgroup, or one wave for planes of up to 1024 cells, per row; fixed tree; no
 * floating-point atomics): a row's result depends only on its cells, its two neighbour rows, the coordinates and the extents, and
 * repeats bit for bit.  16-byte loads when nx and every batch stride are multiples of 16 bytes / sizeof(fg_real) and every field pointer
 * is 16-byte aligned, scalar loads otherwise.  A non-finite value in any channel of a row (a non-finite cell of row y reaches rows y - 1
 * and y + 1 through d/dy) makes the sample, hence the accumulators, of that row NaN and nothing else.  Asynchronous on `stream`; nothing
 * returns to the host.  FG_ERR_INVALID_ARG: a null pointer, n_fields neither 4 nor 7, batch <= 0, an extent below 2, a batch stride
 * below nz * ny * nx, nz * nx above 2^30 or batch * ny above 2^31 - 1. */
int fg_plane_budgets(const fg_real* const* fields, const int64_t* batch_stride, int32_t n_fields, int32_t batch, int32_t nz, int32_t ny,
                     int32_t nx, const double* x, const double* y, const double* z, int32_t wrap_x, int32_t wrap_z, double* n,
                     double* mean, double* central, uint64_t* tickets, void* stream);
/* ---- online wavenumber spectra of wall-parallel planes (csrc/fg_planespectra.hip; both libraries, handle-free) -----------------
 * One sample of PlaneSpectra (simulation/plane_spectra.py; the reference's PSDOnline_Torch, online_statistics.py:269-416): for every
 * slab (env, channel k, listed plane j) the unnormalised DFT of the real plane [nz, nx] over (z, x) -- the convention of
 * numpy.fft.fftn; over x alone when nz = 1 -- of which |u^| is ADDED to amp and |u^|^2 to power, in ONE launch.
 *   channels, batch_stride, K   as for fg_plane_moments (HOST tables, copied into the kernel arguments), K = 1..5
 *   planes           HOST table of n_planes = 1..32 row indices in [0, ny); duplicates are allowed; a caller that wants the mirrored
 *                    plane lists ny - 1 - p as one more entry
 *   amp, power       fp64 device arrays [batch][K][n_planes][max(nz / 2, 1)][nx / 2] of running SUMS: modes kz < max(nz / 2, 1),
 *                    kx < nx / 2 (the reference's fft_slice: the Nyquist mode is not recorded).  The caller zeroes both before the
 *                    first sample and counts the samples itself, so that merging two records is an addition.
 * One workgroup owns a slab: its rows are read once (16-byte loads when nx and every batch stride are multiples of 16 bytes /
 * sizeof(fg_real) and every channel pointer is 16-byte aligned), both transform passes run in LDS on fg_real, |u^| and |u^|^2 are
 * evaluated in fp64, and every accumulator element is read and written by exactly one thread: no floating-point atomics, a slab's
 * result depends only on its cells and the extents and repeats bit for bit.  A non-finite cell makes both accumulators of its slab
 * NaN (every mode) and touches nothing else.  Asynchronous on `stream`; nothing returns to the host.
 * FG_ERR_UNSUPPORTED (before any launch): nx not a power of two in 8..512, nz neither 1 nor a power of two in 4..256, or a slab that
 * does not fit in LDS: (max(nx, nz) + nz (nx / 2 + 1) + 8 max(nx, nz, 2048 / c)) c + 16 bytes above 160 KB, c = 2 sizeof(fg_real).
 * 128 x 128 fits in both libraries.  FG_ERR_INVALID_ARG: a null pointer, K outside 1..5, n_planes outside 1..32, a plane index
 * outside [0, ny), a non-positive extent, a batch stride below nz * ny * nx, batch * K * n_planes above 2^31 - 1. */
int fg_plane_spectra(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz, int32_t ny,
                     int32_t nx, const int32_t* planes, int32_t n_planes, double* amp, double* power, void* stream);
/* ---- online PDFs and joint PDFs of wall-parallel planes (csrc/fg_planehist.hip; both libraries, handle-free) ---------------------
 * One sample of PlaneHistograms (simulation/plane_hist.py; the reference records no distributions): for every listed row
 * (env, rows[r]) the histogram over (z, x) of each of K channels and the joint histogram of each listed channel pair, ADDED to
 * running 64-bit counters, in one launch per 256 listed rows.
 *   channels, batch_stride, K   as for fg_plane_moments (HOST tables, copied into the kernel arguments), K = 1..5
 *   rows             HOST table of n_rows = 1..ny row indices in [0, ny), ascending and unique, copied into the kernel arguments
 *   lo, scale        DEVICE arrays [n_rows][K] of fg_real: the lower edge of row r, channel k and bins / (hi - lo)
 *   bins             2..256.  The slot of a value v, evaluated in fg_real with two separately rounded operations (the file is compiled
 *                    with -ffp-contract=off):  t = (v - lo[r][k]) * scale[r][k];  slot = bins + 2 if v is NaN, 0 if !(t >= 0) (below
 *                    the range, -inf), bins + 1 if t >= bins (at or above the upper edge, +inf), 1 + (int)t otherwise.  t is compared
 *                    as a real before the conversion.
 *   pairs            HOST table [n_pairs][2] of channel indices in [0, K), n_pairs = 0..6; (k, k) is allowed
 *   joint_bins       2..64, a divisor of bins.  A cell whose slots a, b of a pair are both in 1..bins adds one to element
 *                    ja * joint_bins + jb of the pair's slab, j = (slot - 1) / (bins / joint_bins); any other cell adds one to the
 *                    slab's last element ("outside").  The joint table is consistent with the marginals by construction.
 *   counts           DEVICE [batch][n_rows][K][bins + 3]: slot 0 below, 1..bins the bins, bins + 1 above, bins + 2 NaN
 *   joint            DEVICE [batch][n_rows][n_pairs][joint_bins^2 + 1]; NULL exactly when n_pairs == 0
 * The caller zeroes both arrays before the first sample and counts the samples itself, so that merging two records is an addition.
 * Ownership and loads are those of fg_plane_moments (one workgroup, or one wave for planes of up to 1024 cells, per listed row; 16-byte
 * loads under the same conditions).  The sample's histograms are 32-bit counters in LDS, filled with LDS integer atomics; every
 * non-zero one is then added to its global counter by a plain load and store of the row's single owner: every update is an integer
 * addition, no global atomic exists, a row's result depends only on its cells and the tables and repeats bit for bit.  A non-finite
 * cell goes to its slot and harms nothing else; rows and envs that are not listed are not written.  Asynchronous on `stream`; nothing
 * returns to the host.
 * FG_ERR_UNSUPPORTED (before any launch): the counters of a row, K (bins + 3) + n_pairs (joint_bins^2 + 1) words of 4 bytes, do not
 * fit in 160 KB of LDS -- four rows share a workgroup's LDS when the plane has up to 1024 cells, so there 16 bytes per word count.
 * K = 5, bins = 256, n_pairs = 3 fits with joint_bins = 64 for larger planes and with joint_bins = 32 for those.
 * FG_ERR_INVALID_ARG (before any launch): a null pointer or joint != NULL disagreeing with n_pairs, K outside 1..5, bins outside 2..256,
 * joint_bins outside 2..64 or not a divisor of bins, n_pairs outside 0..6, a pair index outside [0, K), n_rows outside 1..ny, rows not
 * ascending and unique or outside [0, ny), a non-positive extent, a batch stride below nz * ny * nx, nz * nx above 2^30 or
 * batch * n_rows above 2^31 - 1. */
int fg_plane_histogram(const fg_real* const* channels, const int64_t* batch_stride, int32_t K, int32_t batch, int32_t nz, int32_t ny,
                       int32_t nx, const int32_t* rows, int32_t n_rows, const fg_real* lo, const fg_real* scale, int32_t bins,
                       const int32_t* pairs, int32_t n_pairs, int32_t joint_bins, uint64_t* counts, uint64_t* joint, void* stream);
int fg_profile_enable(fg_handle h, int on);
int fg_profile_kinds(void);
const char* fg_profile_kind_name(int kind);
int fg_profile_read(fg_handle h, int kind, double* ms_sum, int64_t* samples, double* bytes_sum, double* flops_sum,
                    double* full_ms_sum, double* full_bytes_sum, int64_t* full_samples, int64_t* launches,
                    double* all_ms_sum, int64_t* all_samples);

/* ---- observation resampling -------------------------------------------------------
 * SampleTransformedGridLocalToGlobalMulti + _FillEmptyCells (extensions/resampling.cu:191-609; Python entry
 * sample_multi_coords_to_uniform_grid, pict/data/resample.py:254-358) for ONE rectilinear block, as a gather.
 * The caller supplies, per axis x, y(, z), the continuous output index of every source cell centre split into
 * floor (base) and fraction (frac), concatenated over the axes (lengths n_src[0] + n_src[1] (+ n_src[2])); the
 * index map must be non-decreasing along each axis (it is for the reference's AABB transforms on a rectilinear
 * block).  quirk3d != 0 reproduces the compiled kernel's 6-of-8 corner loop in 3-D (resampling.cu:320), 0 is the
 * full multilinear splat of the reference's pure-torch implementation (resample.py:361-548).
 * fg_resample: src [batch, channels, (nz,) ny, nx] -> dst [batch, channels, (oz,) oy, ox], both fp32 device
 * pointers, channels <= 8; fill_max_steps as fillMaxSteps (resampling.cu:242-290). */
/* Multi-block resampling = a fixed sparse operator per mesh (the folded splat + normalise + hole-fill chain of
 * SampleTransformedGridLocalToGlobalMulti + _FillEmptyCells, resampling.cu:191-609, built on the host once).  y[m][r] = sum_k w * x[m][idx]:
 * ELL rows of equal length K (sensor pixels: the observation of every env step) or CSR (whole render grid).  x: [m][n] device,
 * y: [m][rows] device; index / weight arrays on the device. */
int fg_sparse_apply_ell(const int32_t* idx, const float* w, int32_t rows, int32_t K, const float* x, int64_t n, int32_t m, float* y,
                        void* stream);
int fg_sparse_apply_csr(const int32_t* indptr, const int32_t* col, const float* val, int32_t rows, const float* x, int64_t n, int32_t m,
                        float* y, void* stream);
typedef struct fg_resampler_state* fg_resampler;
int fg_resampler_create(int dims, const int32_t* n_src, const int32_t* n_out, const int32_t* base_cat,
                        const float* frac_cat, int quirk3d, int device, fg_resampler* out);
int fg_resampler_destroy(fg_resampler r);
int fg_resample(fg_resampler r, const float* src, int batch, int channels, float* dst, int fill_max_steps,
                void* stream);

/* ---- RGB frames of the envs of a batch (fp32 library only; csrc/fg_frames.hip) ----------------------------------
 * The last step of the reference's _get_render_data / _format_render_data (envs/fluid_env.py:710-747): one plane of a field, oriented,
 * normalised, clipped, looked up in a 256-entry colour table, solid pixels blacked out, as uint8 RGB.  One launch per 64 listed envs, an
 * env that is not listed costs nothing, nothing returns to the host, no atomics.
 *   field  device fp32 [B][C][nz][ny][nx] (nz == 1 for a 2-D view)
 *   spec   channel >= 0: that channel; -1: the Euclidean norm over all C channels, sqrtf(((u0 u0) + (u1 u1)) + (u2 u2))
 *          axis -1: the 2-D field (rows y, cols x; needs nz == 1, index 0); 0: z = index, rows y, cols x; 1: y = index, rows z, cols x;
 *          2: x = index, rows z, cols y.  Then transpose (rows <-> cols), then flip_rows, flip_cols of the transposed plane: H, W.
 *   table  device uint8 [256][3];  mask: device uint8 [H][W] in output orientation or NULL, non-zero = solid pixel
 *   range  device fp32 [n][2] = (lo, span) of listed env i;  envs: HOST int32 [n], each in [0, B), any order, repeats allowed
 *   out    device uint8 [n][H][W][3]
 * Per pixel, in fp32 with every operation rounded on its own: x = (v - lo) / span (IEEE division); x < 0 -> 0, x > 1 -> 1; NaN -> (0, 0, 0);
 * else table[min((int)(x * 256), 255)]; a masked pixel is (0, 0, 0): byte for byte what matplotlib's
 * cmap(clip((d - vmin) / (vmax - vmin), 0, 1), bytes=True)[..., :3] gives for a float32 array.
 * Before any launch (and without a GPU): FG_ERR_INVALID_ARG for a null field / spec / table / range / envs / out, n < 1, an extent < 1,
 * an env outside [0, B), channel outside [-1, C), an unknown axis, axis -1 with nz != 1, index outside the axis. */
typedef struct fg_frame_spec {
    int32_t channel;
    int32_t axis;
    int32_t index;
    int32_t transpose;
    int32_t flip_rows;
    int32_t flip_cols;
} fg_frame_spec;
int fg_frame_colorize(const float* field, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, const fg_frame_spec* spec,
                      const uint8_t* table, const uint8_t* mask, const float* range, const int32_t* envs, int32_t n, uint8_t* out,
                      void* stream);

/* ---- 3-D frames of the envs of a batch: ray-cast iso-surfaces and volumes (fp32 library only; csrc/fg_render3d.hip) ----------
 * The reference's render(render_3d=True) (envs/util/visualization.py:211-475: marching cubes + Poly3DCollection, ax.voxels) as one ray
 * marcher: one thread per pixel, 16 x 16 pixel tiles, one launch per 64 listed envs, nothing returns to the host, no atomics.
 *   volume   device fp32 [B][C][nz][ny][nx], samples at the integer points of index space, the box [0, nx-1] x [0, ny-1] x [0, nz-1]
 *   channel  >= 0: that channel; -1: the Euclidean norm over all C channels, formed as fg_frame_colorize forms it
 *   camera   an affine ray generator in index space, (x, y, z) per vector: pixel (i, j) (row, column) has the origin
 *            o0 + (j + 1/2) ou + (i + 1/2) ov and the direction d0 + (j + 1/2) du + (i + 1/2) dv (orthographic: du = dv = 0;
 *            perspective: ou = ov = 0); the direction is not normalised, t counts in its units
 *   options  step (in t; samples at t0 + s step), ambient and diffuse of the headlight ambient + diffuse |n.d| / (|n| |d|), the clip box
 *            [clip_lo, clip_hi] of index space for the surface (has_clip != 0), body and background colour
 *   table    device uint8 [256][3];  range: device fp32 [n][2] = (lo, span) of listed env i;  envs: HOST int32 [n], each in [0, B)
 *   out      device uint8 [n][H][W][3]
 * fg_render_isosurface: the first pair of consecutive samples, both inside the clip box, between which |f| - level changes sign, one
 *   secant step, the analytic gradient of the trilinear interpolant as the normal, the colour of color_volume [B][color_C][nz][ny][nx]
 *   at the cell the hit truncates to, normalised by range and looked up as fg_frame_colorize does; level: device fp32 [n]; solid:
 *   device uint8 [nz][ny][nx] or NULL, a second level set at 1/2 along the whole ray, drawn in the body colour, the nearer hit wins;
 *   depth: device fp32 [n][H][W] or NULL, t of the hit or +inf.
 * fg_render_volume: front-to-back emission-absorption over the same samples: bin k of the normalised value, C += (1 - A) opacity[k]
 *   table[k], A += (1 - A) opacity[k], stops once A > 0.99, the rest is the background; opacity: device fp32 [256], per step.
 * The order of the float32 operations is written once at the top of csrc/fg_render3d.hip; the result is defined by it, bit for bit.
 * Limits: a ray takes at most 65536 samples (s = 0 .. 65535): with a step below (path through the box) / 65535 the march ends before
 *   the far side of the box, without an error.  The camera entries are checked one by one; a camera whose sums o0 + (j + 1/2) ou +
 *   (i + 1/2) ov overflow float32 gives positions that are not numbers: such a sample reads cell 0, its value is NaN and crosses nothing.
 * Before any launch (and without a GPU): FG_ERR_INVALID_ARG for a null argument, n < 1, an extent < 2, an env outside [0, B), a channel
 * outside [-1, C), H or W < 1, a frame of 2^31 bytes or more, step <= 0, an empty clip box, a non-finite camera entry, d0 = 0. */
typedef struct fg_render_camera {
    float o0[3], ou[3], ov[3];
    float d0[3], du[3], dv[3];
} fg_render_camera;
typedef struct fg_render_options {
    float step;
    float ambient;
    float diffuse;
    int32_t has_clip;
    float clip_lo[3];
    float clip_hi[3];
    uint8_t body_color[4];      /* r, g, b, unused */
    uint8_t background[4];      /* r, g, b, unused */
} fg_render_options;
int fg_render_isosurface(const float* volume, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, int32_t channel,
                         const float* level, const float* color_volume, int32_t color_C, int32_t color_channel, const float* range,
                         const uint8_t* table, const uint8_t* solid, const fg_render_camera* camera, const fg_render_options* options,
                         int32_t H, int32_t W, const int32_t* envs, int32_t n, uint8_t* out, float* depth, void* stream);
int fg_render_volume(const float* volume, int32_t B, int32_t C, int32_t nz, int32_t ny, int32_t nx, int32_t channel, const float* range,
                     const uint8_t* table, const float* opacity, const fg_render_camera* camera, const fg_render_options* options,
                     int32_t H, int32_t W, const int32_t* envs, int32_t n, uint8_t* out, void* stream);

/* ---- counter-based Gaussian noise on observations / actions of a batch (fp32 library only; csrc/fg_obsnoise.hip) ----------
 * dst[r][i] = src[r][i] + sigma z for every segment (one tensor of an observation dict each), row r < rows and element i < n, in ONE
 * launch; z is normal number i % 4 of the Philox4x32-10 block with
 *   key      (seed & 0xffffffff, seed >> 32)
 *   counter  ((tag << 24) | (i / 4), row_id(r), counters[r][0], counters[r][1])
 * so a row's noise is a pure function of (seed, row id, its episode and step words, tag, element): it does not depend on the batch around
 * it, and the only state is the caller's counters.  The fp32 arithmetic that turns the words into z is written once at the top of
 * csrc/fg_obsnoise.hip and defines the result bit for bit (tests/obs_noise_ref.py restates it in NumPy).
 *   seg       HOST array of n_seg segments (copied into the kernel arguments): src, dst device pointers of `dtype`; src_stride, dst_stride
 *             in elements between rows; n contiguous elements per row; tag < 256; sigma.  dst == src is allowed, any other overlap is not
 *   dtype     0: float, dst = src + (float)sigma * z in fp32;  1: double, dst = src + sigma * (double)z in fp64 (an fp64 env's tensors go
 *             through this entry of the fp32 library); z itself is always formed in fp32
 *   counters  device uint32 [rows][2] = (episode, step);  row_ids: device int32 [rows], or NULL: row r is r
 * Asynchronous on `stream`, no LDS, no atomics, nothing returns to the host.
 * Before any launch (and without a GPU): FG_ERR_INVALID_ARG for a null seg / counters / src / dst, n_seg outside [1, 8], rows outside
 * [1, 65535], an unknown dtype, n outside [1, 2^26], tag >= 256, a stride smaller than n. */
typedef struct fg_noise_segment {
    const void* src;
    void* dst;
    int64_t src_stride, dst_stride;
    int32_t n;
    uint32_t tag;
    double sigma;
} fg_noise_segment;
int fg_obs_noise_add(const fg_noise_segment* seg, int32_t n_seg, int32_t rows, int32_t dtype, uint64_t seed,
                     const uint32_t* counters, const int32_t* row_ids, void* stream);

/* ---- running normalisation of observations and rewards of a batch (fp32 library only; csrc/fg_obsnorm.hip) ----
 * A row is one space-shaped item.  Every statistic slot keeps the record (n, mean, M2): n rows merged so far, a HOST integer passed by
 * value, mean and M2 fp64 on the device.  One update with the selected rows R (m = |R|), all in fp64, every operation rounded on its own:
 *   mean_b = sum_{r in R} x[r] / m;  M2_b = sum_{r in R} (x[r] - mean_b)^2                       (two passes)
 *   delta = mean_b - mean_a;  n = n_a + m;  mean = mean_a + delta * (m / n);  M2 = M2_a + M2_b + delta^2 * (n_a * m / n)
 *   (n_a = 0: the record's memory is not read, the merge returns the batch)
 * and every row, selected or not, is normalised with the record after the update:
 *   rstd = 1 / sqrt(M2 / n + epsilon);  y = (x - mean) * rstd, clipped to [-clip, clip] where clip > 0, rounded once to `dtype`.
 * fg_obs_normalize
 *   seg       HOST array of n_seg segments (copied into the kernel arguments), one tensor of an observation dict each: src, dst device
 *             pointers of `dtype`; src_stride, dst_stride in elements between rows; n contiguous elements per row; mean, m2 device
 *             double [n] (pooled = 0: one slot per element) or [1] (pooled = 1: one slot per key over rows and elements, whose count
 *             is n_rows * n).  dst == src is allowed, any other overlap is not
 *   dtype     0: float, 1: double (an fp64 env's tensors go through this entry of the fp32 library)
 *   n_before  rows in the record before the call; n_add: rows this call merges (m when update != 0, else 0)
 *   row_list  device int32 [n_rows_sel] of ascending rows, or NULL: all rows;  update: 0 only normalises (the record is not written)
 *   Element slots, updating or frozen: the whole dict is ONE launch; statistics, merge and normalisation of a column happen in the
 *   workgroup that owns it.  Pooled slots while updating take one launch more (reduce and merge, then normalise).
 * fg_obs_return_normalize: G[r] = gamma * G[r] + reward[r] (G fp64 [rows] on the device), the update above of the one scalar record
 *   stats = {mean, M2} (device double [2]) with R = every G of this call, and out[r] = reward[r] * rstd (no mean subtraction), clipped
 *   where clip > 0.  One workgroup, one launch.  update = 0 only scales; G still advances.
 * Order rule: the order of every sum is a function of (m, n, pooled) alone -- each lane adds its rows in ascending order, the lanes of
 * a wave combine by the xor butterfly, the waves in ascending order (written out at the top of csrc/fg_obsnorm.hip) -- not of the
 * load form (16-byte words where bases, pitches and n allow, single elements otherwise: the same bits), the addresses or the timing.
 * No floating-point atomic.  Asynchronous on `stream`; nothing returns to the host, nothing is allocated.
 * Before any launch (and without a GPU) FG_ERR_INVALID_ARG: a null pointer, n_seg outside [1, 8], rows outside [1, 65535], n outside
 * [1, 2^26], a stride smaller than n, an unknown dtype, n_add that is not the number of rows the call merges, n_before < 0,
 * update == 0 with n_before == 0, n_rows_sel outside [1, rows] when a list is given, epsilon <= 0, gamma outside [0, 1]. */
typedef struct fg_norm_segment {
    const void* src;
    void* dst;
    int64_t src_stride, dst_stride;
    int32_t n;
    int32_t pooled;
    double* mean;
    double* m2;
} fg_norm_segment;
int fg_obs_normalize(const fg_norm_segment* seg, int32_t n_seg, int32_t rows, int32_t dtype, int64_t n_before, int64_t n_add,
                     const int32_t* row_list, int32_t n_rows_sel, int32_t update, double epsilon, double clip, void* stream);
int fg_obs_return_normalize(const void* reward, void* out, double* G, double* stats, int32_t rows, int32_t dtype, double gamma,
                            int64_t n_before, double epsilon, double clip, int32_t update, void* stream);

/* ---- baseline controllers of the TCF and RBC envs (csrc/fg_baselines.hip; both libraries, handle-free) -------------------------
 * One action of the whole batch in ONE launch each (fluidgym_amd/baselines.py).  Fields are read in place:
 * cell (env, z, y, x) is v[env * batch_stride + (z * ny + y) * nx + x] (batch_stride in reals, >= nz * ny * nx; 2-D: nz = 1).
 * fg_baseline_opposition: v = the wall-normal velocity.  For env b, wall w (n_walls = 1 or 2) and row r = rows[w] (HOST table, like
 *   gain; both copied into the kernel arguments): m = mean of v over the plane (z, x) at y = r, P[i][j] = mean of v over the patch
 *   x in [i actor, (i + 1) actor), z in [j actor, (j + 1) actor) of that plane (one z row per patch where nz = 1), and
 *   action[b][w][i][j] = gain[w] (P[i][j] - m), action [batch][n_walls][nx / actor][nz / actor] on the device.
 * fg_baseline_pd: v = the vertical velocity, wy [ny] DEVICE weights that sum to 1.  E[b][hz][hx] = sum_y wy[y] * mean of v over
 *   x in [hx seg, (hx + 1) seg), z in [hz seg, (hz + 1) seg) (z = 0 alone where nz = 1), and action[b][hz][hx] =
 *   -(kp E + kd_over_dt (E - e_state[b][hz][hx])), the second term 0 for an env with first[b] != 0; then e_state := E and first[b] := 0.
 *   e_state (fp64) and action are [batch][nz / seg][nx / seg] on the device (nz / seg = 1 where nz = 1), first [batch] int32 on the
 *   device.  tickets [batch]: 64-bit device counters, zeroed once by the caller, that order the one write of first[env] after the
 *   reads of it by the env's heaters (an integer atomic, as in fg_plane_moments).
 * Sums are fp64 in a fixed tree -- every lane its cells in ascending order, the xor butterfly of the wave, the waves in ascending
 * order; opposition control sums the plane as the sum of its patch sums -- and the result is rounded once to fg_real: no
 * floating-point atomic, so an env's action depends neither on the launch order nor on the rest of the batch and repeats bit for
 * bit.  One workgroup per (env, wall); one workgroup, or one wave for heater columns of up to 1024 cells, per (env, heater).  16-byte
 * loads where the extents, the pointer and the batch stride allow, single reals otherwise, with the same arithmetic.  Asynchronous
 * on `stream`; nothing returns to the host.  Before any launch (and without a GPU) FG_ERR_INVALID_ARG: a null pointer, batch < 1, a
 * non-positive extent, actor / seg < 1 or not dividing nx (and nz where nz > 1), n_walls not 1 or 2, a row outside [0, ny), a batch
 * stride below nz * ny * nx, a plane or heater column of more than 2^30 cells, more than 2^31 - 1 workgroups. */
int fg_baseline_opposition(const fg_real* v, int64_t batch_stride, int32_t batch, int32_t nz, int32_t ny, int32_t nx,
                           const int32_t* rows, const double* gain, int32_t n_walls, int32_t actor, fg_real* action, void* stream);
int fg_baseline_pd(const fg_real* v, int64_t batch_stride, int32_t batch, int32_t nz, int32_t ny, int32_t nx, int32_t seg,
                   const double* wy, double kp, double kd_over_dt, double* e_state, int32_t* first, uint64_t* tickets,
                   fg_real* action, void* stream);

/* ---- point probes and Lagrangian tracers on a single-block grid (csrc/fg_tracers.hip; both libraries, handle-free) -------------
 * Both entry points share one interpolant of the cell-centred fields of a stretched rectilinear grid (fluidgym_amd/simulation/
 * tracers.py).  fg_point_grid is a HOST record, read during the call: the fields are read in place, cell
 * (env, c, z, y, x) of the velocity is velocity[env * velocity_stride + ((c * nz + z) * ny + y) * nx + x], the boundary velocities
 * bvel[f] (f = 2 * axis + side, NULL on periodic axes) have extent 1 along their normal axis, as for fg_env_restore_field.
 *   nodes[a]   DEVICE array of the axis' nodes: the n cell centres on a periodic axis; the low face, the n centres and the high face
 *              (n + 2) on a FIXED one.  lo[a], len[a]: the low face and the length of the box along the axis.
 * A position is wrapped into [lo, lo + len) on a periodic axis (the interval between the last and the first centre spans the seam) and
 * clamped to [nodes[0], nodes[n + 1]], the face nodes, on a FIXED one; its interval is found by an integer binary search over the node array, staged in LDS,
 * and clamped to a valid interval before any load -- a NaN compares false everywhere and lands in interval 0; a position becomes an
 * index in no other way.  The value is the multilinear blend of the 2^d corners (x, then y, then z) with w = (x - node_i) /
 * (node_i+1 - node_i) and a + w (b - a), b itself at w == 1.  A centre node reads the field; a face node reads, for the velocity, that
 * face's bvel at the corner's other indices (the first axis in the order y, x, z where a corner is a face node on several) and, for
 * the extra fields, the adjacent cell.
 * fg_point_sample: out[env][p][0..d) = the velocity, out[env][p][d + k] = extra[k] (HOST tables of n_extra <= 8 device pointers to
 *   [batch][nz][ny][nx] fields and their batch strides, e.g. pressure and a scalar channel) at points[env * points_env_stride + p * d
 *   + a]; points_env_stride = 0: one point set for all envs.
 * fg_tracer_advect: `substeps` midpoint steps of h = dt / substeps in the frozen field, x* = x + h/2 u(x), x <- x + h u(x*), for the
 *   n_tracers tracers of every env (pos, seed_pos [batch][n][d], age [batch][n], wraps [batch][n][d] int32, lost [batch] uint32).
 *   After every sub-step: a non-finite position respawns (position := seed position, wraps := 0, age := 0 at the end of the call)
 *   and adds 1 to lost[env] (an integer atomic); else, per axis: a periodic axis wraps the position and adds the signed number of
 *   crossings to wraps, so that pos + wraps * len is the unwrapped path; beyond a FIXED face whose bit f is set in respawn_faces the
 *   tracer respawns; beyond any other FIXED face the position is clamped to the face.  age grows by dt per call.
 * One thread per point / tracer, grid (ceil(n / 256), batch); an env's tracers read that env's fields alone, there is no
 * floating-point atomic, so a result depends neither on the batch nor on the launch order and repeats bit for bit.  Asynchronous on
 * `stream`; nothing returns to the host.  Before any launch (and without a GPU) FG_ERR_INVALID_ARG: a null pointer, dims not 2 or 3,
 * a non-positive extent (nz != 1 in 2-D), a periodic flag that is not 0 / 1, a non-finite lo or a len that is not positive and
 * finite, a missing bvel on a FIXED axis, substeps < 1, n_points / n_tracers < 1, n_extra outside 0..8, batch outside 1..65535, a
 * stride smaller than its field, a respawn bit of a face the grid does not have, a non-finite dt, more than 2^30 cells per env;
 * FG_ERR_UNSUPPORTED: node arrays of more than 32 KiB. */
typedef struct fg_point_grid {
    int32_t dims, batch, nx, ny, nz;     /* nz = 1 in 2-D */
    int32_t periodic[3];                 /* x, y, z */
    const fg_real* nodes[3];
    fg_real lo[3], len[3];
    const fg_real* velocity;
    int64_t velocity_stride;
    const fg_real* bvel[6];
    int64_t bvel_stride[6];
} fg_point_grid;
int fg_point_sample(const fg_point_grid* g, const fg_real* const* extra, const int64_t* extra_stride, int32_t n_extra,
                    const fg_real* points, int64_t points_env_stride, int32_t n_points, fg_real* out, void* stream);
int fg_tracer_advect(const fg_point_grid* g, fg_real dt, int32_t substeps, uint32_t respawn_faces, const fg_real* seed_pos,
                     fg_real* pos, fg_real* age, int32_t* wraps, uint32_t* lost, int32_t n_tracers, void* stream);

/* ---- point probes and Lagrangian tracers on a curvilinear multi-block mesh (csrc/fg_mb_tracers.hip; both libraries, handle-free) --
 * One interpolant for the three entry points (fluidgym_amd/simulation/mb_tracers.py).  fg_mb_point_mesh is a
 * HOST record, read during the call; its tables are DEVICE arrays built once by the host (mb_tracers.build_point_tables):
 *   cell_vert [n_cells][2^d]      merged vertex ids of a cell's corners (corner k: bit 0 = x, bit 1 = y, bit 2 = z)
 *   cell_xyz  [n_cells][2^d][d]   the corners' positions as the cell's own block stores them
 *   neighbors [2d][n_cells]       the neighbour cell across face f = 2 * axis + side, or -1 - slot on a FIXED face
 *   face_code [2d][n_cells]       0, or 1 + 2 s (+ 1): crossing the face shifts the position by -shifts[s] (by +shifts[s]) and adds
 *                                 +1 (-1) to the crossing count s
 *   vel_idx, vel_w   [n_vertices][kv]   the velocity stencil of a vertex in ELL form (a weight of 0 is padding; an index >= n_cells
 *                                       names boundary slot index - n_cells);  cell_idx, cell_w [n_vertices][kc]: cell-only fields
 *   shifts[3 s + a]  the n_shifts <= 4 periodic vectors;  slack: the resolution of the local coordinates, in (0, 0.25)
 * The fields are read in place: velocity[env * velocity_stride + c * n_cells + cell], bvel[env * bvel_stride + c * bvel_comp_stride
 * + slot].  A vertex value is sum_k w_k phi_k in table order; the value at (cell, xi) is the multilinear blend of the 2^d vertex
 * values (x, then y, then z; a + w (b - a), b itself at w == 1).
 * fg_mb_point_locate: walks from start_cell (clamped to 0..n_cells-1) to the cell of points[env * points_env_stride + p * d + a]
 *   (points_env_stride = 0: one point set and one start_cell[n_points] for all envs; else n_points * d and start_cell[batch][n_points]):
 *   Newton on the cell map from xi = 1/2 (at most 8 iterations, iterates clamped to [-1, 2]^d, stop below slack / 4); inside where
 *   xi in [-slack, 1 + slack]^d; else through the most violated face that has a neighbour; at most max_walk cell changes.
 *   cell_out, status_out [batch][n_points], xi_out [batch][n_points][d] (clamped to [0, 1]^d).  status 0: found; 1: outside (every
 *   violated face is FIXED: the point stays in that cell); 2: not found (walk exhausted, or a NaN).
 * fg_mb_point_sample: out[env][p][0..d) = the velocity, out[env][p][d + k] = extra[k] (HOST tables of n_extra <= 8 device pointers to
 *   [batch][n_cells] fields and their batch strides) at cell[env * cell_env_stride + p], xi[(env * cell_env_stride + p) * d + a]; the
 *   cell index is clamped to 0..n_cells-1 and xi to [0, 1]^d (a NaN: 0) before any load.  One launch, no walk.
 * fg_mb_tracer_advect: `substeps` midpoint steps of h = dt / substeps in the frozen field for the n_tracers tracers of every env
 *   (pos, seed_pos [batch][n][d]; cell, seed_cell [batch][n]; age [batch][n]; wraps [batch][n][n_shifts] int32; lost [batch] uint32;
 *   respawn_slots uint8 [max(n_slots, 1)]).  x* = x + h/2 u(x) is located from the tracer's cell, x + h u(x*) from there, each by a walk of
 *   at most 64 cell changes.  A walk that ends at a FIXED face puts the tracer on the face (the cell map at the clamped xi), or, where
 *   respawn_slots[slot] != 0, back to its seed (position, cell, wraps := 0, age := 0 at the end of the call); a non-finite position
 *   or an exhausted walk does the same and adds 1 to lost[env] (an integer atomic).  A respawn ends the call for the tracer.
 * One thread per point / tracer, grid (ceil(n / 256), batch), no LDS, no floating-point atomic: an env's result does not depend on
 * the batch and repeats bit for bit.  Asynchronous on `stream`; nothing returns to the host.  Before any launch (and without a GPU)
 * FG_ERR_INVALID_ARG: a null pointer, dims not 2 or 3, batch outside 1..65535, n_cells outside 1..2^28, a negative count, slack outside
 * (0, 0.25), a non-finite shift or dt, a stride smaller than its field, n_points / n_tracers / substeps < 1, n_extra outside 0..8;
 * FG_ERR_UNSUPPORTED: kv or kc above 16, more than 4 shift vectors. */
typedef struct fg_mb_point_mesh {
    int32_t dims, batch, n_cells, n_slots, n_vertices, kv, kc, n_shifts;
    const int32_t* cell_vert;
    const fg_real* cell_xyz;
    const int32_t* neighbors;
    const uint8_t* face_code;
    const int32_t* vel_idx;
    const fg_real* vel_w;
    const int32_t* cell_idx;
    const fg_real* cell_w;
    fg_real slack;
    fg_real shifts[12];
    const fg_real* velocity;
    int64_t velocity_stride;
    const fg_real* bvel;
    int64_t bvel_stride, bvel_comp_stride;
} fg_mb_point_mesh;
int fg_mb_point_locate(const fg_mb_point_mesh* mesh, const fg_real* points, int64_t points_env_stride, int32_t n_points,
                       const int32_t* start_cell, int32_t max_walk, int32_t* cell_out, fg_real* xi_out, int32_t* status_out, void* stream);
int fg_mb_point_sample(const fg_mb_point_mesh* mesh, const fg_real* const* extra, const int64_t* extra_stride, int32_t n_extra,
                       const int32_t* cell, const fg_real* xi, int64_t cell_env_stride, int32_t n_points, fg_real* out, void* stream);
int fg_mb_tracer_advect(const fg_mb_point_mesh* mesh, fg_real dt, int32_t substeps, const uint8_t* respawn_slots, const fg_real* seed_pos,
                        const int32_t* seed_cell, fg_real* pos, int32_t* cell, fg_real* age, int32_t* wraps, uint32_t* lost,
                        int32_t n_tracers, void* stream);

/* ---- env glue either side of the n sim steps of an env step (fp32 library only) ------------------------------
 * fg_envglue_jet_schedule: the action smoothing of the reference's jet envs (cylinder_env_base.py:748-753, a_k = a_{k-1} +
 * alpha (target - a_{k-1}) before every sim step) for the n sim steps of one env step at once: control[k][b] = target[b] +
 * (current[b] - target[b]) * decay[k] (decay[k] = (1 - alpha)^(k+1), device array of n), jets[k][wall][b][c][0][x] =
 * shape[c][x] * control[k][b] (two walls, two components, nx % 4 == 0), last[b] = control[n-1][b].  The slabs are what
 * fg_multi_step binds as the wall velocities of sim step k.
 * fg_envglue_channel_observe: what step() returns after them (fluid_env.py:749-800) for the channel env: cross[b] = mean(v^2),
 * shear[b] = shear_scale * (mean_x u[y=0] + mean_x u[y=ny-1]), reward[b] = -(shear + penalty * cross), the sensor gather
 * obs_velocity[b][s][c] = velocity[b][c][sensor[s]], obs_pressure[b][s] = pressure[b][sensor[s]] (sensor: flat cell indices,
 * int64, device).  One workgroup per env and a fixed summation tree: an env's result does not depend on the batch. */
int fg_envglue_jet_schedule(const float* target, const float* current, const float* decay, const float* shape, int32_t n,
                            int32_t batch, int32_t nx, float* jets, float* last, void* stream);
int fg_envglue_channel_observe(const float* velocity, const float* pressure, const int64_t* sensor, int32_t n_sensors,
                               int32_t batch, int32_t ny, int32_t nx, float shear_scale, float penalty, float* obs_velocity,
                               float* obs_pressure, float* cross, float* shear, float* reward, void* stream);
/* The same with env b's own shear scale: shear_scale_B = device array [batch] (per-env viscosities, fg_set_viscosity_batch). */
int fg_envglue_channel_observe_batch(const float* velocity, const float* pressure, const int64_t* sensor, int32_t n_sensors,
                                     int32_t batch, int32_t ny, int32_t nx, const float* shear_scale_B, float penalty,
                                     float* obs_velocity, float* obs_pressure, float* cross, float* shear, float* reward,
                                     void* stream);

/* ---- multi-block, non-orthogonal domains -------------------------------------------
 * The reference's general Domain: several structured blocks of curvilinear cells (vertex coordinates ->
 * CoordsToTransforms, grid_gen.cu:298-390), joined by ConnectedBoundary with shuffled / inverted axes
 * (Block::ConnectBlock, domain_structs.cpp:1940-1950; ConnectBlocks :1080-1113), closed by FIXED Dirichlet
 * boundaries (Block::CloseBoundary :1995-2002) or periodic (Block::MakePeriodic :1952-1971), stepped by
 * _PISO_split_step's non-orthogonal branch (PISOtorch_simulation.py:1707-1972) with
 * nonOrthoFlags = CENTER_MATRIX | DIRECT_MATRIX | DIAGONAL_RHS (:479-487).  This is what the cylinder and airfoil
 * environments run on (envs/cylinder/grid.py:232-418).
 *
 * Build: fg_mb_create -> fg_mb_add_block per block (HOST vertex coordinates [d,(nz+1,)ny+1,nx+1], float32;
 * every face starts FIXED with zero velocity) -> fg_mb_connect / fg_mb_make_periodic -> fg_mb_finalize (builds the
 * mesh tables on the host once, allocates work space).  Faces are numbered -x,+x,-y,+y,-z,+z = 0..2d-1; the
 * connected-axis arguments use the same numbering with the low bit meaning "inverted", exactly as ConnectBlock.
 * Cells of all blocks are concatenated (block order, x fastest): N = fg_mb_sizes; the FIXED faces of all blocks are
 * concatenated into NB boundary slots (block order, face order, lowest remaining axis fastest); fg_mb_block_info
 * gives the offsets.  Fields are caller-owned fp32 device arrays: velocity [B,d,N] (updated in place), pressure
 * result [B,N] (read for the lagged corner terms, overwritten with the new mean-free pressure), boundary velocity
 * [B,d,NB] (Dirichlet values, may change between steps), optional velocity source [B,d,N].
 * fg_mb_set_reference_quirks (before finalize; default 1,1) keeps two behaviours of the reference that are not
 * geometrically motivated: diagonal walks over a connection land one layer inside the connected block
 * (PISO_multiblock_cuda_kernel.cu:2152, 2658, 2825), and the matrices drop the cross-metric terms on the inner face
 * of a first-layer cell when the far side of the block is a wall (:1952). */
typedef struct fg_mb_state* fg_mb_handle;
int fg_mb_create(int32_t dims, int32_t batch, int32_t device, fg_mb_handle* out);
int fg_mb_destroy(fg_mb_handle h);
int fg_mb_add_block(fg_mb_handle h, const fg_real* vertex_coords_host, int32_t nx, int32_t ny, int32_t nz, int32_t* block_id);
int fg_mb_connect(fg_mb_handle h, int32_t block1, int32_t face1, int32_t block2, int32_t face2, int32_t axis1, int32_t axis2);
int fg_mb_make_periodic(fg_mb_handle h, int32_t block, int32_t axis);
int fg_mb_set_reference_quirks(fg_mb_handle h, int32_t connected_diagonal_offset, int32_t first_layer_rule);
/* nonOrthoFlags of the reference (PISOtorch_simulation.py:479-487), before finalize: 25 = CENTER_MATRIX | DIRECT_MATRIX |
 * DIAGONAL_RHS, what Simulation(non_orthogonal=True) runs (default); 10 = DIRECT_RHS | DIAGONAL_RHS: every cross-metric term
 * lagged on the right-hand side, which leaves the pressure matrix symmetric with the exact constant null space */
int fg_mb_set_nonortho_flags(fg_mb_handle h, int32_t flags);
int fg_mb_finalize(fg_mb_handle h);
int fg_mb_sizes(fg_mb_handle h, int32_t* n_cells, int32_t* n_boundary_faces);
int fg_mb_block_info(fg_mb_handle h, int32_t block, int32_t* cell_offset, int32_t* boundary_slot0 /* [2d], -1 = not FIXED */);
int fg_mb_get_neighbors(fg_mb_handle h, int32_t* out_host /* [2d*N]: neighbour cell, or -1 - boundary slot */);
/* Every mesh table the kernels read (csrc/fg_mb.h), as built on the host: 0 nbr, 1 fcode, 2 T, 3 Tb, 4 bcell, 5 bface, 6 Vdiag,
 * 7 Voff, 8 KPp, 9 KPn, 10 SVc_idx, 11 SVc_w, 12 SVb_idx, 13 SVb_w, 14 SP_idx, 15 SP_face, 16 SP_wp, 17 SP_wn (4-byte elements;
 * out may be NULL to query the count).  A handle created with device < 0 is host-only: it builds and serves these tables
 * without touching a GPU (CPU parity tests of the topology code), every compute entry point refuses it. */
int fg_mb_get_host_table(fg_mb_handle h, int32_t which, void* out, int64_t* count);
int fg_mb_bind(fg_mb_handle h, fg_real* velocity, fg_real* pressure_result, fg_real* boundary_velocity, const fg_real* source);
int fg_mb_set_viscosity(fg_mb_handle h, fg_real nu);
/* One viscosity per env: caller-owned device array [batch], read by the step's kernels at launch (the values may be rewritten
 * between steps); NULL returns to the scalar.  Every entry must be > 0 (checked here on a host copy: FG_ERR_INVALID_ARG). */
int fg_mb_set_viscosity_batch(fg_mb_handle h, const fg_real* nu_B);
typedef struct fg_mb_step_options {
    int32_t corrector_steps;           /* 2 */
    int32_t advect_non_ortho_steps;    /* 1 (airfoil 2) */
    int32_t pressure_non_ortho_steps;  /* 1 (cylinder 3-D and airfoil 4) */
    int32_t max_iterations;            /* 5000 */
    fg_real advection_tol;               /* RMS residual */
    fg_real pressure_tol;
    int32_t pressure_use_bicgstab;     /* 0: CG as the reference (pressure_use_BiCG=False, simulation.py:136) -- with the
                                          cross-metric terms the pressure matrix is not symmetric, CG only works while the
                                          mesh is close to orthogonal; 1: BiCGStab (restarted every 200 iterations);
                                          2: BiCGStab with the iterate kept in fp64 and the residual recomputed in fp64 at every
                                          restart (iterative refinement), best refinement point returned when unconverged -- the role of
                                          the reference's solver_double_fallback */
    int32_t pressure_warm_start;       /* 1: the first pressure solve of a corrector starts from the current pressure field
                                          instead of zero (the reference passes x=None there, PISOtorch_simulation.py:1878;
                                          same converged answer, fewer iterations) */
    int32_t pressure_project_mean;     /* 1: CG works on residuals with their mean removed -- identical on orthogonal meshes,
                                          and what keeps the solve from stalling on the constant residual component that the
                                          cross-metric terms feed (1^T P != 0); 0: the reference's plain recurrence */
    fg_real pressure_stall_accept;       /* > 1: a CG solve whose best iterate is within this factor of pressure_tol and has
                                          not improved for 20 iterations ends with that iterate: the reference's
                                          pressure matrix has a near-null LEFT vector y that is not constant, so a
                                          flux-balanced right-hand side keeps a component (y.b) y no iteration can remove
                                          -- a residual floor |y.b| / sqrt(N) that sits at 1.1e-5 on the reference's own
                                          cylinder mesh, right at its 1e-5 tolerance; 0: off */
    int32_t solver_double_fallback;    /* the reference's retry ladder (_linear_solve, PISOtorch_diff.py:410-476).  A solve counts as failed
                                          like there: the velocity solve when it did not converge, a pressure solve (returnBestResult)
                                          when its residual is non-finite.  1: a failed solve is repeated from zero with the iterate
                                          kept in fp64 and the residual b - M x recomputed in fp64 at every restart (the reference
                                          repeats it with matrix and vectors cast to fp64) */
    int32_t bicg_precondition_fallback; /* 1: a BiCGStab solve that (still) failed is repeated from zero with a preconditioner: here
                                          right diagonal scaling (M D^-1) y = b, x = D^-1 y -- same residual, same criterion; the
                                          reference's rung is cuSPARSE ILU(0), whose triangular solves are sequential */
} fg_mb_step_options;
/* dt_B: device array [B]; dt <= 0 leaves that env untouched.  stats_host (optional, 4 ints): max iterations of
 * {-, velocity, pressure corrector 0, pressure corrector 1}.  Returns FG_ERR_NOT_CONVERGED / FG_ERR_NOT_FINITE when a
 * solve failed (unconverged: fields updated from the best iterate, as with returnBestResult; non-finite: the envs concerned
 * are left as they were, see fg_mb_env_status), other negative codes on errors. */
int fg_mb_piso_step(fg_mb_handle h, const fg_real* dt_B, const fg_mb_step_options* opt, int32_t* stats_host, void* stream);
/* Per-env outcome of the last fg_mb_piso_step / fg_mb_single_step, host array [B]: 0 ok; 1 a solve of the batch ended
 * unconverged (best iterate used, returnBestResult); 2 a solve of THIS env was non-finite -- its step was not committed
 * (velocity as before the step, like solve_ok=False before CopyVelocityResultToBlocks, PISOtorch_simulation.py:1752-1757,
 * and Simulation.single_step -> False, simulation.py:259-280) while the other envs of the batch completed. */
int fg_mb_env_status(fg_mb_handle h, int32_t* out_B_host);
/* How often each rung of the retry ladder ran since the handle was created: out4 = {velocity fp64 rung, velocity preconditioned
 * rung, pressure fp64 rung, pressure last-resort CG}.  force_mask (tests): bit 0 / bit 1 make the FIRST attempt of every
 * velocity / pressure solve count as failed, so that the rungs can be exercised on systems that do not fail. */
int fg_mb_ladder(fg_mb_handle h, int64_t* out4_host, int32_t force_mask);
/* Tuning aid: with FG_MB_OC_VARIANT=256 in the environment at fg_mb_create, workgroup 0 of the on-chip CG counts shader-clock
 * cycles per phase of its loop; out12 = 11 phases + iterations of the last launch. */
int fg_mb_debug_cycles(fg_mb_handle h, uint64_t* out12_host);
/* What a handle remembers between solves besides the bound fields: where the previous solve of each place in the step finished
 * (its next solve polls there first; a verified / refined BiCGStab re-opens and restarts at its polls, so the schedule is part of
 * the arithmetic), the back-off state of the multilevel trial and (round 6) the back-off of the velocity sweeps -- skip, failures,
 * sweeps per non-orthogonal pass -- which decides whether a solve runs the sweeps or BiCGStab.  get_state / set_state of the envs
 * carry these 48 words so that a restored state replays bit for bit (reference: envs/fluid_env.py:1320-1363).  set = 0 reads, 1 writes. */
int fg_mb_solver_hints(fg_mb_handle h, int32_t* hints48, int32_t set);
/* A multi-block handle has no per-env restore (its flat cell order has no mirror or roll): both return FG_ERR_UNSUPPORTED. */
int fg_mb_env_restore_field(fg_mb_handle h, int which_field, const fg_real* bank, int32_t S, const fg_env_sel* sel, int32_t n_sel,
                            int32_t signed_components, void* stream);
int fg_mb_env_reset_solver_state(fg_mb_handle h, const fg_env_sel* sel, int32_t n_sel, void* stream);
/* ---- per-env restore of a multi-block handle from a bank of stored states (csrc/fg_mb_envrestore.hip) ----
 * A multi-block handle carries three per-env arrays between steps -- velocity [B][d][N], pressure [B][N] and the boundary velocity
 * [B][d][NB] -- and ONE launch restores all three for every record of sel (the records of fg_env_restore_field; flip_x and shift_x
 * must be 0): env `env` becomes state `src` of the banks, mirrored (flip_z) and then rolled (shift_z) along the span.  The span is a
 * symmetry of the topology when the handle is 3-D and every block is z-periodic with one nz (whether the layers are equally thick is
 * the caller's business: simulation/mb_state_bank.span_symmetry); on every other handle flip_z and shift_z must be 0 and the restore
 * is a copy.  The cells of a block, cell_offset + (z ny + y) nx + x, and the slots of a FIXED x- or y-face, slot0 + z len + t, are
 * segments {first, plane, nz}, and on both
 *     dst[first + z plane + r] = sign(c) bank[src][first + zs plane + r],  zs = flip_z ? nz-1 - ((z - shift_z) mod nz) : (z - shift_z) mod nz
 * with sign(c) = -1 for component 2 of the velocity and of the boundary velocity under flip_z, else +1: per block and per face
 * torch.roll(torch.flip(t, [z]), shift_z, z).  Envs not named in sel are not written.
 * noise (NULL: every value is a copy or a negation): counter-based Gaussian reset noise on velocity (sigma_velocity) and pressure
 * (sigma_pressure), none on the boundary values.  Destination cell i of component tag c (0..d-1 velocity, d pressure) takes normal
 * i % 4 of the Philox4x32-10 block with key (seed low, seed high) and counter ((c << 24) | (i / 4), env, episodes[k], 0xFFFFFFFF) for
 * record k -- the stream of fg_obs_noise_add with a step word that the observation noise never reaches -- and dst = value +
 * (float)sigma z in the fp32 library, value + sigma (double)z in the fp64 one.  It depends on (seed, env, episode, c, i) only: not on
 * the batch, nor on the other records of the call.
 * sel and noise->episodes are HOST arrays [n_sel]; they are checked here, uploaded in one copy to an array the handle owns and read by
 * the one launch; the call is asynchronous on `stream`.  Every check comes before any launch and before the bound-field check, so a
 * host-only handle (device < 0) answers every refusal.  FG_ERR_INVALID_ARG: a null handle, sel or bank (bank_boundary may be NULL
 * when NB == 0), S < 1, n_sel outside 1..B, an env out of range or named twice, src outside [0, S), a non-zero flip_x or shift_x, a
 * flip that is not 0 / 1, shift_z outside [0, nz), flip_z or shift_z where the span is no symmetry of the topology, a sigma that is
 * negative or not finite.  FG_ERR_UNSUPPORTED: noise with N > 2^26 (the first counter word).  FG_ERR_NOT_BOUND: the handle is not
 * finalised or has no bound fields. */
typedef struct fg_mb_reset_noise {
    uint64_t seed;
    double sigma_velocity, sigma_pressure;
    const uint32_t* episodes;  /* host [n_sel] */
} fg_mb_reset_noise;
int fg_mb_restore_envs(fg_mb_handle h, const fg_real* bank_velocity /*[S][d][N]*/, const fg_real* bank_pressure /*[S][N]*/,
                       const fg_real* bank_boundary /*[S][d][NB], may be NULL when NB == 0*/, int32_t S, const fg_env_sel* sel,
                       int32_t n_sel, const fg_mb_reset_noise* noise /*NULL: pure copy*/, void* stream);
/* ---- per-env unsteady inflow of a multi-block handle: gusts (csrc/fg_mb_inflow.hip) ----
 * ONE launch, one workgroup per env: the inflow slots [slot0, slot0 + count) of every env b are rewritten from a base profile (an
 * array in the layout of the boundary velocity, [B][d][NB]) and that env's gust signals at t = n dt, n = counters[b][0] * sim_steps
 * + k:
 *     ub[b][0][s] = base[b][0][s] * (1 + S_b),   ub[b][1][s] = base[b][1][s] + base[b][0][s] * G_b(y[s]),   ub[b][c >= 2][s] = base
 *     S_b = sum_k a_k sin 2 pi (f_k t + phi_k),   G_b(y) = sum_k g_k sin 2 pi (h_k t + psi_k - kappa y)
 * then the signed boundary fluxes of the env are summed over all NB slots and, where their sum exceeds 0.01 outflow_tol, the up to
 * two outflow ranges are scaled by -fixed / free (the balance rule of the step's PRE hook; its advective update is not run).  The
 * phases in double, the signals in fp32 by a rule of separately rounded operations written at the top of the source file and
 * restated in tests/inflow_disturbance_ref.py.  signal[b] = (S_b, G_b(y_mid)).
 * modes: a device table [B][6][8] of doubles, rows a, f, phi, g, h, psi (n_streamwise / n_transverse of the 8 columns are read), or
 * NULL: the random form, whose modes are a pure function of (seed, env_offset + b, counters[b][1]) -- Philox4x32-10 with key
 * (seed low, seed high) and counter ((240 << 24) | k, env_offset + b, counters[b][1], 0); f_k and h_k fall into the k-th of
 * n_streamwise / n_transverse equal parts of [f_lo, f_hi], every a_k = streamwise_rms sqrt(2 / n_streamwise), every g_k =
 * transverse_rms sqrt(2 / n_transverse).  n_streamwise = n_transverse = 0 writes the base profile back and rebalances.
 * Every pointer of the struct is a DEVICE pointer; nothing is read back; asynchronous on `stream`.  Every check comes before the
 * launch: FG_ERR_INVALID_ARG for a null handle, struct or pointer (modes may be NULL), a mode count outside 0..8, count <= 0, slots
 * out of range or overlapping, outflow_count <= 0, a dt that is negative or not finite, sim_steps < 1, k outside [0, sim_steps), a
 * non-finite kappa, y_mid or outflow_tol and, in the random form, a band that is not 0 <= f_lo <= f_hi < inf or an rms that is
 * negative or not finite; FG_ERR_NOT_BOUND for a handle that is not finalised or has no bound fields. */
typedef struct fg_mb_inflow_params {
    int32_t slot0, count;                                                    /* the inflow slots */
    int32_t outflow_slot0, outflow_count, outflow_slot0_b, outflow_count_b;  /* the outflow ranges (the second may be empty) */
    int32_t n_streamwise, n_transverse;                                      /* K_s, K_t in 0..8 */
    int32_t sim_steps, k;                                                    /* sim steps per env step, index of this one */
    int32_t env_offset, reserved;
    uint64_t seed;
    double dt, f_lo, f_hi, streamwise_rms, transverse_rms, kappa, y_mid, outflow_tol;
    const void* base;          /* [B][d][NB] of fg_real */
    const double* y;           /* [count] face centres */
    const double* modes;       /* [B][6][8] or NULL */
    const uint32_t* counters;  /* [B][2] = (env steps of the episode, episode) */
    float* signal;             /* [B][2] */
} fg_mb_inflow_params;
int fg_mb_inflow_disturbance(fg_mb_handle h, const fg_mb_inflow_params* params, void* stream);
/* as fg_solver_counters, for the multi-block path */
int fg_mb_solver_counters(fg_mb_handle h, int64_t* out13_host, int32_t reset);
/* The tuning / diagnosis switches a handle runs under (the FG_* environment variables read ONCE at create time, docs/SWITCHES.md,
 * and the solver policies set through the API), as one JSON object written to buf (NUL-terminated, at most n bytes; returns the
 * length needed when the buffer is too small, a negative status on error).  bench.py stores it with every result, so a number can
 * be traced to the code paths that produced it.  (No counterpart in the reference: its solver has no such switches.) */
int fg_config_dump(fg_handle h, char* buf, int n);
int fg_mb_config_dump(fg_mb_handle h, char* buf, int n);
/* What a handle created NOW would read from the environment: {variable: value} for every switch of a family (0 single-block,
 * 1 multi-block), parsed by the rules of the switch table; needs no device.  Same buffer convention as the dumps. */
int fg_switch_values(int32_t family, char* buf, int32_t n);
int fg_mb_solver_unconverged(fg_mb_handle h, int64_t* out4_host);   /* as fg_solver_unconverged */
/* Simulation.single_step for such a domain (simulation.py:206-280): boundary-flux guard, per-env adaptive substeps
 * (_PISO_adaptive_step, PISOtorch_simulation.py:2004-2064), the advective-outflow PRE hook on ONE FIXED face given as
 * a range of boundary slots (update_advective_boundaries + balance_boundary_fluxes, :188-393; count 0 = none) and
 * fg_mb_piso_step per substep.  out_host as for fg_single_step: [0..3] max solver iterations of the last substep,
 * [4] substeps taken, [5] 1 if every solve converged; flux_host (optional, [B]) the boundary flux balance found. */
typedef struct fg_mb_sim_options {
    fg_mb_step_options step;
    fg_real time_step;
    fg_real cfl;
    int32_t adaptive;          /* 1: substeps from the CFL condition; 0: `substeps` equal steps */
    int32_t substeps;
    fg_real flux_balance_tol;
    int32_t outflow_slot0;
    int32_t outflow_count;
    fg_real outflow_velm[3];     /* characteristic velocity of the convective condition */
    fg_real outflow_tol;         /* tol of update_advective_boundaries (balance threshold = 0.01 tol) */
    int32_t max_substeps;      /* safety bound, 0 = none */
    int32_t outflow_slot0_b;   /* a second outflow face (the airfoil mesh has two: airfoil/grid.py:708-714); count 0 = none */
    int32_t outflow_count_b;
} fg_mb_sim_options;
int fg_mb_single_step(fg_mb_handle h, const fg_mb_sim_options* opt, int32_t* out_host, fg_real* flux_host, void* stream);
/* the PRE hook alone, same dt for every env (make_divergence_free runs it with dt = 1, PISOtorch_simulation.py:1334-1345) */
int fg_mb_update_advective_boundary(fg_mb_handle h, fg_real dt, int32_t slot0, int32_t count, int32_t slot0_b, int32_t count_b,
                                    const fg_real* velm, fg_real tol, void* stream);
/* Simulation.make_divergence_free (PISOtorch_simulation.py:1318-1429), without its PRE hook */
int fg_mb_make_divergence_free(fg_mb_handle h, const fg_mb_step_options* opt, void* stream);
/* Domain.GetBoundaryFluxBalance per env; synchronises */
int fg_mb_boundary_flux_balance(fg_mb_handle h, fg_real* out_B_host, void* stream);
/* host copies of the mesh tables: per boundary slot the owner cell, its face and Minv | det of the face
 * (k_CoordsToFaceTransforms, grid_gen.cu:398-470); per cell Minv | det (k_CoordsToTransforms, :298-354) */
int fg_mb_get_boundary_tables(fg_mb_handle h, int32_t* cell, int32_t* face, fg_real* transform);
int fg_mb_get_cell_transforms(fg_mb_handle h, fg_real* transform);
/* max |Minv u| over cells and boundary faces per env (Domain.getMaxVelocity(True, True)); synchronises */
int fg_mb_max_velocity(fg_mb_handle h, fg_real* out_B_host, void* stream);
/* fg_flow_diagnostic on a multi-block domain: out[B, K, N] in the flat cell order, g[i][j] = sum_a c[i][a] Minv[a][j] with the cell's
 * Minv; across a connection only the neighbour's VALUE is used (no axis mapping), across a FIXED face the slot's boundary velocity.
 * Same kinds and codes; a host-only handle (created with device < 0) answers FG_ERR_UNSUPPORTED. */
int fg_mb_flow_diagnostic(fg_mb_handle h, int kind, fg_real* out, void* stream);
/* pressure_project_mean keeps the CG residuals orthogonal to a unit vector: the constant by default, or y_host [N] (any scale).
 * fg_mb_unit_pressure_matrix leaves the pressure matrix for A = 1 in the P buffers so that a host routine can compute its left
 * near-null vector, the choice that removes the residual floor of non-orthogonal meshes */
int fg_mb_set_residual_projection(fg_mb_handle h, const fg_real* y_host);
/* Iterations a CG solve may go without improving its kept iterate before it ends with that iterate (default 400;
 * the reference has no such limit: its solves run to maxIterations and return the best result,
 * cg_solver_kernel.cu:345-361, PISOtorch_diff.py:266-371). */
int fg_mb_set_stall_limit(fg_mb_handle h, int32_t iterations);
/* Start vector of the first velocity solve of a step: 0 (default of a new handle) zero, the reference's non-orthogonal branch
 * (x=None at no_step 0, PISOtorch_simulation.py:1735-1742); 1 the current velocity (opt-in: fewer iterations, same answer within
 * the tolerance).  Later non-orthogonal passes always start from the previous pass's result as there. */
int fg_mb_set_advection_start(fg_mb_handle h, int from_result);
/* fg_mb_set_advection_jacobi(on): the velocity systems by point-Jacobi sweeps over the neighbour table (mb_jacobi, csrc/fg_mb_krylov.hip)
 * before the reference's BiCGStab (bicgstab_solver_kernel.cu:63-411 at PISOtorch_simulation.py:1735-1742) -- the single-block policy
 * `advection_jacobi` on the multi-block path: same systems, same criterion; a system the sweeps do not contract on (the airfoil meshes)
 * is handed to BiCGStab from a cleared start vector after the first check.  fg_mb_advection_jacobi_counts: solves settled by the
 * sweeps, solves handed on. */
int fg_mb_set_advection_jacobi(fg_mb_handle h, int on);
int fg_mb_advection_jacobi_counts(fg_mb_handle h, int64_t* out2);
/* Additive multilevel preconditioner of the pressure solves on 2-D meshes: Jacobi + 1/2 x Jacobi on 4 x 4 aggregates + the
 * dense pseudo-inverse on 8 x 8 aggregates, all from the geometry-only (A = 1) matrix and scaled per env.  Host arrays: a4 [N]
 * (aggregate of every cell), parent4 [n4] (8 x 8 aggregate of every 4 x 4 one), rect4 (every 4 x 4 aggregate as a rectangle of
 * cells of one block; checked against a4), d4g [n4], aci8 [n8 x n8]; n4 < 65535, n8 <= 2048.  Consumers: the on-chip CG
 * (k_mbc_onchip; up to 16 k cells, n4 <= 2048, n8 <= 512) applies it inside the persistent kernel, the pressure BiCGStab of any
 * mesh takes it as right preconditioner in kernel form (three launches per application).  a4 == NULL only switches it on / off
 * (enable).  The reference's CG / BiCGStab run without one (cg_solver_kernel.cu; its ILU0 is the fallback rung only); converged
 * answers agree to the solver tolerance, iteration counts drop 3-9x.
 * Both builds: in the fp64 build (fg_real = double) the tables arrive as doubles, the layouts of the fp32 on-chip / cluster kernels
 * are left out, the pressure CG applies the preconditioner in kernel form (five launches per iteration, mb_cg) and the pressure
 * BiCGStab takes the unfused apply. */
int fg_mb_set_multilevel(fg_mb_handle h, int32_t n4, int32_t n8, const int32_t* a4_host, const int32_t* parent4_host,
                         const int32_t* rect4_host /* [n4][4]: first cell, width, height, row stride */, const fg_real* d4g_host,
                         const fg_real* aci8_host, fg_real geom_diag_sum, int32_t enable);
/* Stress harness of the multi-block velocity BiCGStab: solves the d systems per env held in the assembly buffers (FG_MB_BUF_A,
 * _C_OFF, _RHS, e.g. loaded from a dumped failing step) `reps` times from zero; out4 = solves, solves with a non-finite system,
 * unconverged solves, max iterations; acc_out / sc_out receive the recurrence words (accumulators, alpha / omega) as the last solve
 * left them.  Debugging aid (profiles/bicg_stress.py), not on any step path. */
int fg_mb_debug_bicgstab(fg_mb_handle h, fg_real tol, int32_t max_iterations, int32_t reps, int64_t* out4,
                         double* acc_out /* [B d][12] or NULL */, fg_real* sc_out /* [B d][2] or NULL */, void* stream);
/* z = M r [B,N] with the kernel form of the multilevel preconditioner on the pressure matrix currently assembled (unit test of
 * the three kernels behind the preconditioned pressure BiCGStab; synchronises). */
int fg_mb_multilevel_apply(fg_mb_handle h, const fg_real* r_BN, fg_real* z_BN, void* stream);
/* One pressure CG solve, from zero, of the systems held in the pressure buffers (FG_MB_BUF_P_DIAG / _P_OFF, right-hand side
 * FG_MB_BUF_DIV) under whatever fg_mb_set_multilevel has switched on; per env: iterations, converged (and finite), final RMS residual.
 * Test entry (synchronises), both builds; an unconverged solve is reported through the outputs, not as an error. */
int fg_mb_debug_pressure_cg(fg_mb_handle h, fg_real tol, int32_t max_iterations, int32_t project_mean, int32_t* iterations_B,
                            int32_t* converged_B, double* residual_B, void* stream);
/* z = U^-1 L^-1 r [B,d,N] with ILU(0) of the velocity matrix assembled by the last step: the preconditioner of the multi-block
 * BiCG_precondition_fallback rung (cuSPARSE ILU(0) in the reference, bicgstab_solver_kernel.cu:191-226; level-scheduled on the
 * mesh's neighbour table here).  Test entry (synchronises); FG_ERR_UNSUPPORTED in the fp64 build and on meshes in which a cell
 * meets the same neighbour across two faces (the rung keeps right diagonal scaling there). */
int fg_mb_debug_ilu_apply(fg_mb_handle h, const fg_real* r_BdN, fg_real* z_BdN, void* stream);
/* The multilevel right preconditioner of the pressure BiCGStab is a trial with exponential back-off per handle:
 * out3 = current back-off in solves (0: no tables; 4: every attempt converges; up to 256), attempts, failed attempts (each repeated
 * with the plain recurrence). */
int fg_mb_multilevel_status(fg_mb_handle h, int32_t* out3);
/* Force on a closed wall from the bound fields: replaces the tensor arithmetic of the reference's envs/util/forces.py
 * (compute_forces_2d :193-276, compute_forces_3d :278-377) behind CylinderEnvBase._get_drag_and_lift (cylinder_env_base.py:676-700).
 * cell_index / slot_index [layers][n]: the wall-adjacent cell and the boundary slot of every wall face in ring order (device);
 * geom [5][n]: outward normal x, y, tangential spacing, wall distance, face length (device); out [B][2][layers] (device) =
 * sum over the ring of ((2 nu S - p I) n) * face length * area_scale.  Asynchronous on `stream`. */
int fg_mb_wall_forces(fg_mb_handle h, const int32_t* cell_index, const int32_t* slot_index, const fg_real* geom, int32_t n,
                      int32_t layers, fg_real area_scale, fg_real viscosity, fg_real* out, void* stream);
/* The same with env b's own viscosity: viscosity_B = device array [batch] read at launch, or NULL for `viscosity` in every env. */
int fg_mb_wall_forces_batch(fg_mb_handle h, const int32_t* cell_index, const int32_t* slot_index, const fg_real* geom, int32_t n,
                            int32_t layers, fg_real area_scale, fg_real viscosity, const fg_real* viscosity_B, fg_real* out,
                            void* stream);
int fg_mb_unit_pressure_matrix(fg_mb_handle h, void* stream);
/* live timing of the CG kernel pair (kind 0: stencil kernel k_mbc_ap, 1: update kernel k_mbc_update): every fourth chunk of
 * iterations has its first pair issued with start/stop events; sums over sampled launches with live systems, their
 * ALGORITHMIC bytes (active systems x cells x per-cell figure) and the total launches since enable */
int fg_mb_profile_enable(fg_mb_handle h, int32_t on);
const char* fg_mb_profile_kind_name(int32_t kind);
int fg_mb_profile_read(fg_mb_handle h, int32_t kind, double* ms_sum, int64_t* samples, double* bytes_sum, int64_t* launches);
/* kind 2 = k_mbc_onchip, the CG that runs a whole solve of one env inside one workgroup (meshes up to 28 672 cells, 2-D):
 * every launch is timed; bytes = what it streams from L2 / Infinity Cache (off-diagonals + packed neighbour table per
 * iteration and cell); fg_mb_profile_iterations = CG iterations summed over envs and solves since enable */
int fg_mb_profile_iterations(fg_mb_handle h, int64_t* iterations);
#define FG_MB_BUF_A 0               /* [B,N]   diagonal of C */
#define FG_MB_BUF_C_OFF 1           /* [B,2d,N] */
#define FG_MB_BUF_RHS 2             /* [B,d,N] velocity right-hand side of the last solve */
#define FG_MB_BUF_H 3               /* [B,d,N] */
#define FG_MB_BUF_DIV 4             /* [B,N]   pressure right-hand side of the last solve */
#define FG_MB_BUF_P_DIAG 5
#define FG_MB_BUF_P_OFF 6
#define FG_MB_BUF_VELOCITY_RESULT 7
#define FG_MB_BUF_KRYLOV0 8          /* 8..12: the five Krylov work vectors [B,d,N] as the last solve left them (debugging) */
#define FG_MB_BUF_PRESSURE_X 13     /* [B,N]   the iterate x of the last pressure solve as the solver left it (fg_mb_debug_pressure_cg:
                                     * untouched; a PISO step's mean removal subtracts the mean in place before it copies to the bound pressure) */
int fg_mb_get_buffer(fg_mb_handle h, int32_t which, const fg_real** ptr, int64_t* count);
int fg_mb_read_buffer(fg_mb_handle h, int32_t which, fg_real* dst_device, void* stream); /* device copy, synchronises */

/* ---- grid metrics --------------------------------------------------------------------------- */
/* CoordsToTransforms (grid_gen.cu:298-390): vertex coords [d,(nz+1,)ny+1,nx+1] ->
 * transforms [(nz,)ny,nx, 2 d^2 + 1] = M | Minv | det per cell. */
int fg_coords_to_transforms(const float* coords, float* transforms, int dims, int nx, int ny, int nz,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDGYM_HIP_H */
