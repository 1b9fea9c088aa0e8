"""Generates docs/SWITCHES.md: every environment switch of the package.  The native ones come from the text of their one table
(fluidgym_amd/csrc/fg_switches.h), those read in Python from the os.environ sites, annotated in NOTES.  A getenv / os.environ site
without a row, or a row without a site (a native handle switch's table entry IS its site), fails the run, so the table cannot rot:
    python profiles/gen_switch_table.py            # rewrite docs/SWITCHES.md
    python profiles/gen_switch_table.py --check    # exit 1 if the committed table is stale (tests/test_switch_table.py)"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = os.path.join("fluidgym_amd", "csrc", "fg_switches.h")
ENTRY = re.compile(r'X\((FG_\w+), ([\w.]+), (-?\d+), (\w+), (HANDLE|PROCESS), (no|bits|policy), "(.*)"\)')

# switches read in Python: name -> (changes results?, what it does).  "bits" = same converged answer, different rounding / iteration trajectory;
# "no" = timing / diagnosis only; "policy" = a documented departure from (or return to) the reference's solver policy
NOTES = {
    "FLUIDGYM_AMD_ADVECTION_JACOBI": ("policy", "policy advection_jacobi (default 1): the Simulation asks for the Jacobi sweeps of fg_jacobi.hip on the grids that qualify"),
    "FLUIDGYM_AMD_PRESSURE_REFINEMENT": ("bits", "policy pressure_refinement (default 0 = off): up to N mixed-precision corrections behind every single-block pressure solve (fp64 residual, fp32 corrections: fg_set_pressure_refinement) -- an accuracy mode"),
    "FLUIDGYM_AMD_MULTI_STEP": ("no", "0: the sim steps of an env step are issued one by one from Python instead of through fg_multi_step (A/B runs; same bits)"),
    "FLUIDGYM_AMD_F64_FD": ("bits", "0: the fp64 library solves the pressure systems with the reference's plain CG instead of the CG preconditioned by the fast-diagonalisation operator in doubles (csrc/fg_f64_fd.hip; A/B runs: iterations per solve)"),
    "FLUIDGYM_AMD_ENV_GLUE": ("bits", "0: ChannelJet2D's action schedule and reward / observation as elementwise torch launches instead of the two native kernels of fg_envglue.hip (A/B runs; the schedule is bit-identical, the means differ by fp32 rounding of the summation order)"),
    "FLUIDGYM_AMD_LANES": ("no", "default of ParallelFluidEnv(lanes=...): sub-batches of a rank's env batch, each its own solver handle, stepped concurrently by that many host threads on their own HIP streams (1 = one batch; bench.py passes --lanes 2).  Same bits per env as the sub-batches stepped alone"),
    "FG_FD_NO_FFT": ("bits", "1: the x basis change of the FD preconditioner as dense GEMM instead of the row FFT (tests)"),
    "FLUIDGYM_AMD_LIB": ("no", "path of libfluidgym_hip.so (sanitizer build: tests/run_sanitizer_suite.sh)"),
    "FLUIDGYM_AMD_LIB_F64": ("no", "path of libfluidgym_hip_f64.so"),
    "FLUIDGYM_AMD_ADVECTION_FD_PRECONDITIONER": ("bits", "policy advection_fd_preconditioner: auto (2-D periodic-x grids) / always / never"),
    "FLUIDGYM_AMD_ADVECTION_LINE_PRECONDITIONER": ("bits", "policy advection_line_preconditioner (off)"),
    "FLUIDGYM_AMD_ADVECTION_RUNG_PRECONDITIONER": ("bits", "preconditioner of the BiCG_precondition_fallback rung: line / ilu"),
    "FLUIDGYM_AMD_ADVECTION_WARM_START": ("policy", "1: velocity solve starts from the current velocity in both branches (reference: branch rule)"),
    "FLUIDGYM_AMD_PRESSURE_WARM_START": ("policy", "1: pressure solves start from the previous pressure (reference: zero)"),
    "FLUIDGYM_AMD_PRESSURE_STALL_ACCEPT": ("policy", "accept a stalled pressure solve within a factor of the tolerance (off)"),
    "FLUIDGYM_AMD_PRESSURE_MULTILEVEL": ("bits", "multilevel preconditioner of the multi-block pressure CG"),
    "FLUIDGYM_AMD_PRESSURE_MULTILEVEL_BICGSTAB": ("bits", "multilevel trial of the airfoil's refined BiCGStab"),
    "FLUIDGYM_AMD_PRESSURE_MULTILEVEL_FP64": ("bits", "policy pressure_multilevel_fp64 (default 0): float64 cylinder / airfoil envs on 2-D meshes install the multilevel preconditioner in the fp64 build (kernel-form preconditioned CG, unfused BiCGStab trial) instead of the plain recurrences"),
    "FLUIDGYM_AMD_PRESSURE_BICGSTAB_LARGE_MESHES": ("bits", "3-D multi-block ids take the refined BiCGStab"),
    "FLUIDGYM_AMD_NATIVE_WALL_FORCING": ("bits", "policy native_wall_forcing: the TCF forcing hook runs inside the library"),
    "FLUIDGYM_COLLECTIVE_TIMEOUT_S": ("no", "timeout of ParallelFluidEnv's process group (600 s)"),
    "FLUIDGYM_FORCE_COLLECTIVES": ("no", "ParallelFluidEnv issues its collectives at world size 1 too (tests)"),
    "FLUIDGYM_MASTER_PORT": ("no", "rendezvous port of the reference-style ParallelFluidEnv(cuda_ids=...) entry"),
    "FLUIDGYM_DATA_PATH": ("no", "local data path (initial domains), as config.update('local_data_path', ...)"),
}
IGNORE = {"RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY", "PYTHONPATH", "OMP_NUM_THREADS",
          "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "TMPDIR", "GRAFT_REPO_ROOT"}


def native_rows():
    rows = {}      # name -> (results, what, scope, table line) of every entry of the switch table
    for no, line in enumerate(open(os.path.join(ROOT, TABLE)), 1):
        for m in ENTRY.finditer(line):
            rows[m.group(1)] = (m.group(6), m.group(7), m.group(5), f"{TABLE}:{no}")
    return rows


def scan():
    found = {name: [row[3]] for name, row in native_rows().items()}      # (a PROCESS switch needs a getenv site of its own beside it)
    for base, _, files in os.walk(os.path.join(ROOT, "fluidgym_amd")):
        if "_san" in base or "_f64" in base or "_var" in base or "__pycache__" in base:
            continue
        for fn in files:
            if not fn.endswith((".hip", ".h", ".py")):
                continue
            path = os.path.join(base, fn)
            rel = os.path.relpath(path, ROOT)
            for no, line in enumerate(open(path, errors="replace"), 1):
                for m in re.finditer(r'getenv\("([A-Z][A-Z0-9_]+)"\)', line):
                    found.setdefault(m.group(1), []).append(f"{rel}:{no}")
                for m in re.finditer(r'environ(?:\.get)?[\[(]\s*"([A-Z][A-Z0-9_]+)"', line):
                    found.setdefault(m.group(1), []).append(f"{rel}:{no}")
    return {k: v for k, v in found.items() if k not in IGNORE}


def render(found):
    lines = ["# Environment switches of fluidgym_amd", "",
             "Generated by `python profiles/gen_switch_table.py` from the switch table of the native library (`fluidgym_amd/csrc/fg_switches.h`) and the",
             "`os.environ` sites of the Python source; `tests/test_switch_table.py` fails when this file is stale.  The native library reads its handle",
             "switches ONCE, at `fg_create` / `fg_mb_create` (never on a step path), so two handles of one process may run under different values;",
             "`fg_config_dump` / `fg_mb_config_dump` report the values a handle runs under and `bench.py` stores them with every leg",
             "(`profiles/bench_detail.json`).  `FG_HTRACE` and `FG_ROCTX` are process-wide, read when the library is loaded.  None is needed in normal operation.", "",
             "A native value is read as C's `atoi` reads it: optional sign and leading decimal digits, so `01` is 1, and text that does not start with a number",
             "(empty, `off`, `true`) is 0 -- which switches an on-unless-0 switch OFF.  The rule of every switch stands beside it in the table file.", "",
             "*results*: **no** = timing / diagnosis only; **bits** = the same converged answer through another kernel form (rounding and",
             "iteration trajectories differ); **policy** = a documented departure from (or return to) the reference's solver policy.", "",
             "| variable | results | read at | what |", "|---|---|---|---|"]
    notes = {**NOTES, **{name: row[:2] for name, row in native_rows().items()}}
    for name in sorted(found):
        res, what = notes[name]
        where = ", ".join(f"`{w}`" for w in found[name][:2]) + (" ..." if len(found[name]) > 2 else "")
        lines.append(f"| `{name}` | {res} | {where} | {what} |")
    lines += ["", "Build-time defines (profiling builds only): `-DFG_ACC_ACCESS`, `-DFG_FLAG_ACCESS`, `-DFG_MB_OC_CYCLES`, `-DFG_KNOCK_B`, `-DFG_WAVE_SHFL`,",
              "`-DFG_DCT_KNOCK` -- see the comments where they are tested.", ""]
    return "\n".join(lines)


def main():
    found = scan()
    rows = set(NOTES) | set(native_rows())
    missing = sorted(set(found) - rows)
    gone = sorted((rows - set(found)) | {name for name, row in native_rows().items() if row[2] == "PROCESS" and len(found[name]) < 2})
    if missing or gone:
        print(f"switch table out of date: in the source without a note {missing}; noted but not in the source {gone}")
        return 1
    text = render(found)
    path = os.path.join(ROOT, "docs", "SWITCHES.md")
    if "--check" in sys.argv:
        # line numbers move with every edit: compare names and annotations only
        cur = open(path).read() if os.path.exists(path) else ""
        strip = lambda t: re.sub(r"\| `[^|]*:\d+`[^|]*\|", "| |", t)
        return 0 if strip(cur) == strip(text) else 1
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").write(text)
    print(f"wrote {path}: {len(found)} switches")
    return 0


if __name__ == "__main__":
    sys.exit(main())
