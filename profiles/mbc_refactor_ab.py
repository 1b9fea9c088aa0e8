"""A/B of two builds of the library on the chunked multi-block pressure CG (`mbc_refactor_ab.json`: k_mbc_ap / k_mbc_update written
once for one and four cells per thread and for the preconditioned recurrence, iteration index as a launch argument, against the
commit before).  `FLUIDGYM_AMD_LIB` / `FLUIDGYM_AMD_LIB_F64` select the other build; one process per build, run alternately on one
machine in one session.

    rocprofv3 --kernel-trace --stats -d DIR -o t -- python profiles/mbc_refactor_ab.py solve
        the reference's cylinder mesh (make_vortex_street_mesh(24), 14 232 cells, 8 envs) with the on-chip and cluster CG off: the fp32
        library (four cells per thread), the fp64 library (one cell), the fp64 library with the multilevel preconditioner; a random
        mean-free right-hand side on the matrix of one PISO step, solved from zero REPS times each.  Prints `AB {...}` with the
        iterations per solve; the per-kernel averages are rocprofv3's
    python profiles/mbc_refactor_ab.py stats DIR
        calls and average duration of the k_mbc_ap / k_mbc_update instances in DIR's kernel statistics, one JSON line
    python profiles/mbc_refactor_ab.py resources LOG
        VGPRs, SGPRs, scratch, LDS and occupancy of the k_mbc_ap / k_mbc_update instances from the remarks of a compile of
        fg_mb_krylov.hip with -Rpass-analysis=kernel-resource-usage (stderr in LOG), one JSON line
"""
import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 4
KERNEL = re.compile(r"k_mbc_(ap|update)")


def solve():
    import ctypes

    import numpy as np
    import torch

    from fluidgym_amd import _lib as L
    from fluidgym_amd.envs.cylinder_grid import build_domain, make_vortex_street_mesh

    os.environ["FG_MB_ONCHIP"], os.environ["FG_MB_CLUSTER"] = "0", "0"   # read at fg_mb_create
    mesh = make_vortex_street_mesh(24)
    hip = ctypes.CDLL("libamdhip64.so")
    out = {"lib": os.environ.get("FLUIDGYM_AMD_LIB", "in-tree build")}
    for name, dtype, pre, tol in (("f32_w4", torch.float32, False, 1e-6), ("f64_w1", torch.float64, False, 1e-10),
                                  ("f64_w1_pre", torch.float64, True, 1e-10)):
        dom = build_domain(mesh, 0.01, batch=8, dtype=dtype)
        if pre:
            assert dom.set_pressure_multilevel(fp64=True) is not None
        g = torch.Generator(device="cpu").manual_seed(5)
        dom.velocity.copy_((0.3 * torch.randn(dom.velocity.shape, generator=g)).to(dom.device))
        dom.velocity[:, 0] += 1.0
        dom.piso_step(0.01, pressure_tol=1e-6, advection_tol=1e-6, pressure_project_mean=True, raise_on_failure=False)
        rhs = np.random.default_rng(3).standard_normal((8, dom.n_cells))
        rhs = torch.from_numpy(np.ascontiguousarray(rhs - rhs.mean(1, keepdims=True), dom._np)).cuda()
        ptr, cnt = ctypes.c_void_p(), ctypes.c_int64()
        L.check(dom.lib.fg_mb_get_buffer(dom.handle, L.FG_MB_BUF_DIV, ctypes.byref(ptr), ctypes.byref(cnt)))
        assert cnt.value == rhs.numel()
        assert hip.hipMemcpy(ptr, ctypes.c_void_p(rhs.data_ptr()), ctypes.c_size_t(rhs.element_size() * rhs.numel()), 3) == 0
        torch.cuda.synchronize()
        runs = [dom.debug_pressure_cg(tol, 5000, project_mean=True) for _ in range(REPS)]
        out[name] = {"iterations": [r["iterations"] for r in runs], "converged": [all(r["converged"]) for r in runs]}
        dom.close()
    print("AB " + json.dumps(out), flush=True)


def stats(d):
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if KERNEL.search(row["Name"]):
                name = row["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                out[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3)}
    print("STATS " + json.dumps(out, sort_keys=True), flush=True)


def resources(log):
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
    for line in open(log):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark: [^ ]* *([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and name and KERNEL.search(name) and m.group(1).strip() in keys:
            out.setdefault(name, {})[keys[m.group(1).strip()]] = int(m.group(2))
    print("RESOURCES " + json.dumps(out, sort_keys=True), flush=True)


if __name__ == "__main__":
    {"solve": solve, "stats": lambda: stats(sys.argv[2]), "resources": lambda: resources(sys.argv[2])}[sys.argv[1]]()
