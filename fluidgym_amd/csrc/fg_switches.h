// THE table of the library's environment switches: X(variable, handle member, default, parse rule, scope, results class, "what it does").
// Everything else derives from it: the members (FG_SW_MEMBER in fg_state / fg_mb_state), the read at fg_create / fg_mb_create
// (fg_switches_read: the only place a handle switch meets the environment), the switch part of fg_config_dump / fg_mb_config_dump,
// fg_switch_values, and docs/SWITCHES.md (profiles/gen_switch_table.py parses this text: keep every entry on one line).
// Parse rules (fg_switch_parse; a value is read as atoi reads it, so text that is no decimal integer counts as 0):
//     INT  the integer, unset = the default          POS  the integer where it is positive, else the default
//     ON   0 where the integer is 0, else 1          OFF  1 where the integer is not 0, else 0 (unset: 0)
//     ONE  1 where the integer is 1, else 0          SET  1 where the variable exists at all
//     TRI  unset = -1 (by the rule), else 0 / 1      ALL  the integer, unset and 1 = the default (every bit)
// scope: HANDLE = read once per handle at create; PROCESS = read once per process, into a global.  results: as docs/SWITCHES.md says.
#pragma once
#include <string>

enum FgSwitchRule { FG_SW_INT, FG_SW_POS, FG_SW_ON, FG_SW_OFF, FG_SW_ONE, FG_SW_SET, FG_SW_TRI, FG_SW_ALL };
int fg_switch_parse(const char* text, FgSwitchRule rule, int def);

// both handle families (members declared by hand: FgPoll::spin / words, adv_jacobi beside adv_jacobi_env = "the variable was set")
#define FG_COMMON_SWITCHES(X) \
    X(FG_POLL_SPIN, poll.spin, 1, ON, HANDLE, no, "0: host polls wait with hipStreamSynchronize instead of spinning on pinned sequence words") \
    X(FG_POLL_WORDS, poll.words, 1, ON, HANDLE, no, "0: polled verdicts through the host-pinned mirror + a system-scope release (one L2 write-back per verdict kernel) instead of travelling in the 8-byte result words the host spins on (A/B runs: 8 790 against 9 600 env-steps/s on the headline, one lane); reported as 0 where the handle has no result words (fp64 build, FG_POLL_SPIN=0)") \
    X(FG_ADV_JACOBI, adv_jacobi, 0, INT, HANDLE, bits, "velocity systems of uniform 2-D grids and of the multi-block meshes: 1 Jacobi sweeps first (fg_jacobi.hip, mb_jacobi), 0 BiCGStab always; unset = what fg_set_advection_jacobi / fg_mb_set_advection_jacobi says (the Simulation turns it on: policy advection_jacobi)")

// single-block handles (fg_state)
#define FG_SB_SWITCHES(X) \
    X(FG_CG_FUSED, cg_fused, 1, INT, HANDLE, bits, "1 (default): three-launch preconditioned pressure CG on 2-D fast-transform grids (fg_fftcg.hip); 0: the five kernels") \
    X(FG_BICG_PFUSED, bicg_pfused, 1, INT, HANDLE, bits, "1 (default): six-launch Helmholtz-preconditioned BiCGStab (fg_fftbicg.hip); 0: eleven launches per iteration") \
    X(FG_BICG_FUSED, bicg_fused, 1, INT, HANDLE, bits, "1 (default): two-kernel BiCGStab iteration in 2-D; 0: five kernels; 2: two kernels in 3-D bricks too") \
    X(FG_BICG_SUB, bicg_sub, -1, INT, HANDLE, no, "envs per sub-batch of the 2-D two-kernel BiCGStab (unset: by working set; 0: never)") \
    X(FG_BICG3, bicg3_force, -1, INT, HANDLE, bits, "z-marching 3-D BiCGStab (fg_bicgstab3d.hip): 0 never, N always with z-chunk N (tests on small grids), unset: when the grid fits the tiles and fills the chip") \
    X(FG_BICG3_BXL, bicg3_bxl, 0, INT, HANDLE, no, "tile lanes along x of the z-marching BiCGStab (16 / 32)") \
    X(FG_BICG3_MIX, bicg3_mix, 3, INT, HANDLE, bits, "debugging: bit 0 kernel a, bit 1 kernel b as z-march, bit 2 keep the init kernel") \
    X(FG_REDUCE_WGS, reduce_wgs, 0, INT, HANDLE, no, "workgroups per env of the reduction kernels (0 = the rule of fg_reduce_wgs)") \
    X(FG_HELM_ROWFORM, helm_rowform, 1, ON, HANDLE, bits, "0: Helmholtz factors through k_helm_coeffs + the array-form line kernels (IEEE division instead of the hardware reciprocal)") \
    X(FG_ADV_LINESWEEP, adv_linesweep, 0, INT, HANDLE, bits, "1: the advection-diffusion systems of the Helmholtz-preconditioned family (wall-refined 2-D grids: RBC) go to line sweeps x <- (D + O_y)^-1 (b - O_x x) first (k_line_sweep_y, fg_linepre.hip), BiCGStab takes what they do not settle; 0 (default): the preconditioned BiCGStab always -- measured on the RBC leg: 16-17 sweeps per velocity solve at the bench state's sub-step, 775 against 793 env-steps/s") \
    X(FG_FD_FACFUSE, fd_facfuse, 1, INT, HANDLE, no, "1 (default): the first tridiagonal solve after 1/A changed makes the per-env row-mean factors itself (k_tridiag_y_lds<.., FAC>: same arithmetic, same bits); 0: k_fd_rowmean_factor as a launch of its own (A/B runs)") \
    X(FG_FD_ROWMEAN, fd_rowmean, 1, INT, HANDLE, bits, "1 (default): the fused pressure CG is preconditioned by the row-mean operator (per-env factors, one factorisation per PISO step); 0: the grid's A = 1 factors") \
    X(FG_FCG_FIRST, fcg_first, 1, ON, HANDLE, bits, "1 (default): the fused CG judges its first iterate from I'(0)'s dot products (k_fcg_check0) and stores no pressure when every env ends there; 0: the verdict on the updated residual (A/B runs, tests)") \
    X(FG_FCG_SPEC, fcg_spec, 1, ON, HANDLE, no, "0: the corrector waits for the verdict on the first iterate instead of being launched behind the verdict kernel (A/B runs)") \
    X(FG_JAC_SPEC, jac_spec, 1, ON, HANDLE, no, "0: k_h and the divergence kernel of the first corrector wait for the verdict on the velocity sweeps instead of being launched behind the check kernel (A/B runs)") \
    X(FG_JAC_PREFACTOR, jac_prefactor, 1, ON, HANDLE, no, "0: the row-mean factors of the pressure preconditioner are made in front of the first tridiagonal solve instead of behind the sweeps' check kernel (A/B runs)") \
    X(FG_JAC_WARM, jac_warm, -1, TRI, HANDLE, bits, "start vector of the Jacobi sweeps of a step's velocity systems: 1 the block velocity, 0 the BiCGStab start vector (zero on the non-orthogonal branch); unset: the block velocity on on-chip grids of 2^17 cells and more (where it saves a pass)") \
    X(FG_JAC_XCD, jac_xcd, 1, INT, HANDLE, no, "0: the on-chip Jacobi regions in launch order instead of one XCD per run of an env's regions (A/B runs)") \
    X(FG_JAC_SHAPE, jac_shape, 0, INT, HANDLE, bits, "A/B runs of the Jacobi sweeps: 1 full-row regions only, 2 bands only (unset: the cheaper of the two for the grid)") \
    X(FG_JAC_SWEEPS, jac_sweeps, 0, INT, HANDLE, bits, "A/B runs: sweeps per pass of the Jacobi sweeps, clamped to what the region allows (unset: 4 / 6 / 8 for full rows, 8 / 12 for bands, by region depth)") \
    X(FG_FORCE_ZMARCH, zmarch_force, 0, INT, HANDLE, bits, "z-march chunk length of the 3-D Poisson kernels (tests on small grids; -1 = brick kernels)") \
    X(FG_ZMARCH_SB, zmarch_sb, -1, INT, HANDLE, no, "single-barrier ring of the z-march kernels: bit per mode forces it on with the caller's chunk length, 0 never, unset = where the launch is one full round") \
    X(FG_DEV_DT, dev_dt, 1, INT, HANDLE, no, "0: fg_single_step waits for the CFL maxima and computes the adaptive sub-steps on the host before the PISO step, instead of the CFL kernel's last workgroup taking them on the device (FgDtRule: same doubles, same bits) and the host reading the maxima after the step (A/B runs)") \
    X(FG_PROF_PERIOD, prof_period, 64, POS, HANDLE, no, "sampling period of the live kernel timing: every 64th launch of a kind is timed (8 cost the timed region ~5 %: a count kernel + two events per sample)")

// multi-block handles (fg_mb_state); the fp64 build overrides four of them after the read (fg_switches_read)
#define FG_MB_SWITCHES(X) \
    X(FG_MB_BICG_VEC4, dbg_vec_mask, 31, ALL, HANDLE, no, "bit per multi-block BiCGStab kernel: four-cell form (1 p, 2 v, 4 s, 8 t, 16 x; 1 or 31 = all)") \
    X(FG_MB_BICG_FUSE, dbg_fuse_st, 2, INT, HANDLE, bits, "multi-block BiCGStab: 0 five kernels, 1 s/t fused, 2 (default) also p/v") \
    X(FG_MB_ML_FUSE, dbg_ml_fuse, 1, INT, HANDLE, bits, "multilevel BiCGStab forms p / s inside the restriction: 0 never, 1 up to 32 systems, 2 always") \
    X(FG_MB_ML_TRY_CAP, dbg_ml_cap, 200, POS, HANDLE, policy, "iteration cap of an attempt of the multilevel trial (200; tests force 2)") \
    X(FG_MB_TRACE, dbg_trace, 0, SET, HANDLE, no, "residual / verification trace of the pressure BiCGStab on stderr") \
    X(FG_MB_TRACE_FAIL, dbg_fail, 0, SET, HANDLE, no, "recurrence words of a system that ends non-finite") \
    X(FG_MB_COMPACT, dbg_compact, 1, INT, HANDLE, no, "0: every multi-block Krylov launch covers all systems of the batch") \
    X(FG_MB_OC_RTG_NT, oc_rtg_nt, 1024, INT, HANDLE, bits, "register-resident on-chip CG with a global residual copy on 16-24 k-cell meshes instead of k_mbc_l2: workgroup size of that instance (1024 x 24 or 512 x 48 cells per thread)") \
    X(FG_MB_ONCHIP, onchip_mode, 1, ON, HANDLE, bits, "0: no whole-solve on-chip CG (chunked CG kernels)") \
    X(FG_MB_OC_AGG, dbg_oc_agg, 1, ON, HANDLE, bits, "0: cell-ordered on-chip CG instead of the aggregate-owned one") \
    X(FG_MB_OC_VARIANT, oc_variant, 0, INT, HANDLE, no, "on-chip CG variant bits (bit 0: no compiler fences in the stencil pass; bit 1: split [F][N] coefficient layout)") \
    X(FG_MB_CLUSTER, cl_mode, 1, INT, HANDLE, bits, "pressure CG of an env by a cluster of four workgroups (fg_mb_cluster.hip): 0 never (the one-workgroup kernels), 1 (default) meshes beyond 8 k cells, 2 every mesh its tables fit (tests)") \
    X(FG_MB_CL_JACOBI, cl_jacobi, 1, ON, HANDLE, bits, "0: the velocity sweeps of the meshes the cluster CG takes stay one launch per sweep (k_mbj_sweep_env) instead of one launch per solve by the clusters (k_mbj_cluster; A/B runs: 2 552 against 3 045 env-steps/s on the cylinder mesh)") \
    X(FG_MB_CL_HALF, cl_half, 1, ON, HANDLE, bits, "0: meshes whose rows of the coarse inverse do not fit LDS as fp32 stream them from L2 instead of holding them as fp16 (A/B runs: 19.7 against 16.8 us per iteration on 23 k cells)") \
    X(FG_MB_CL_MAXCL, cl_max_clusters, 0, INT, HANDLE, no, "cap on the clusters of one launch of the cluster CG (tests: envs beyond it queue inside the kernel; same bits)") \
    X(FG_MB_CL_NEAR, cl_near, 1, ON, HANDLE, no, "0: granule stores of the cluster CG always write through to memory, also when a cluster's workgroups reported one XCD (A/B runs: 10.0 against 8.6 us per iteration)") \
    X(FG_MB_RUNG_ILU, dbg_rung_ilu, 1, ON, HANDLE, bits, "0: column-scaled preconditioned rung instead of ILU(0)") \
    X(FG_MB_PCG_KERNEL, dbg_pcg_kernel, 0, ONE, HANDLE, bits, "1 (fp32 build, debugging): the multilevel-preconditioned pressure CG as the kernel-form loop of mb_cg (five launches per iteration, `k_mbc_ap<.., MBC_PRE>` / `k_mbc_update<.., true>`: what the fp64 build runs) instead of the on-chip / cluster kernels; 0 (default)")

// process-wide tracers of fg_poll.hip: no handle in reach where they are used, read when the library is loaded (into these globals)
extern int fg_htrace_on, fg_roctx_on;
#define FG_PROCESS_SWITCHES(X) \
    X(FG_HTRACE, fg_htrace_on, 0, OFF, PROCESS, no, "1: host time stamps around the polls and the launches behind them (fg_poll.hip), per-pair averages printed at exit") \
    X(FG_ROCTX, fg_roctx_on, 0, OFF, PROCESS, no, "1: named roctx ranges around the phases of a step (fg_single_step, scalar / velocity assembly and solve, pressure correctors; mb_velocity_solve, mb_pressure_solve) for rocprofv3 --marker-trace; the library is dlopen'ed, off by default")

#define FG_SW_MEMBER(var, member, def, rule, scope, results, what) int member = def;

// the environment into the handle's switch members (fg_create / fg_mb_create, before anything reads one) | "VARIABLE": value for every
// switch of the handle's family, appended to an open JSON object
void fg_switches_read(struct fg_state* s);
void fg_switches_read(struct fg_mb_state* s);
void fg_switches_json(const struct fg_state* s, std::string& json);
void fg_switches_json(const struct fg_mb_state* s, std::string& json);
void fg_json_put(std::string& json, const char* key, long long value);      // one more member of an open JSON object
int fg_json_out(const std::string& json, char* buf, int n);      // the dumps' length rule: FG_OK, or the length needed when n is too small
