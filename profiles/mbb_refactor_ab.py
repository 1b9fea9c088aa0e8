"""A/B of two builds of the library on the multi-block legs of bench.py (`mbb_refactor_ab.json`: the BiCGStab kernels written once
for one and four cells per thread against the commit before).  One process per build -- `FLUIDGYM_AMD_LIB=<other build>/libfluidgym_hip.so`
selects it -- run alternately on one machine in one session; prints one line `AB {...}` with the env-steps/s of the legs.

    python profiles/mbb_refactor_ab.py both           # cylinder_env (64 envs, 6 steps) and airfoil_env (64 envs, 3 steps) as bench.py runs them
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/mbb_refactor_ab.py airfoil_prof    # one short airfoil leg: per-kernel averages
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(0)
what = sys.argv[1] if len(sys.argv) > 1 else "both"
out = {"lib": os.environ.get("FLUIDGYM_AMD_LIB", "in-tree build"), "what": what}
if what in ("both", "cylinder"):
    out["cylinder_env"] = bench.cylinder_env_leg(dev, steps=6, extra_modes=False)["value"]
if what in ("both", "airfoil"):
    out["airfoil_env"] = bench.airfoil_env_leg(dev, num_envs=64, steps=3)["value"]
if what == "airfoil_prof":
    out["airfoil_env"] = bench.airfoil_env_leg(dev, num_envs=64, steps=1, develop=20)["value"]
print("AB " + json.dumps(out), flush=True)
