"""Policy pressure_multilevel_fp64 off against on, same build, same process: CylinderJet2D-easy-v0 in float64, 8 envs, 10 env steps
after 3 warm-up steps per measurement, alternated off / on / on / off over five rounds (ABBA).  Prints one JSON line (medians,
spreads = max - min over the rounds, pressure iterations per solve) and writes it to --out when given.
    python profiles/f64_multilevel_ab.py [--envs 8] [--steps 10] [--warmup 3] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidgym_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="CylinderJet2D-easy-v0")
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    envs, state0 = {}, {}
    for on in (False, True):
        old = fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=on)
        try:
            env = fluidgym_amd.make(a.env, num_envs=a.envs, dtype=torch.float64, initial_domain_steps=3, randomize_initial_state=False)
            env.reset(seed=0)
        finally:
            fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=old["pressure_multilevel_fp64"])
        envs[on], state0[on] = env, env.get_state()
    act = torch.full_like(envs[False]._zero_action, 0.25)

    def measure(on):
        env = envs[on]
        env.set_state(state0[on])
        for _ in range(a.warmup):
            env.step(act)
        env._domain.solver_counters(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            env.step(act)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c = env._domain.solver_counters()
        return dt / a.steps * 1e3, (c["pressure0"]["mean"], c["pressure1"]["mean"]), c["piso_steps"]

    ms, its, piso = {False: [], True: []}, {}, {}
    for r in range(a.rounds):
        for on in ((False, True, True, False) if r % 2 == 0 else (True, False, False, True)):
            t, i, p = measure(on)
            ms[on].append(t); its[on] = i; piso[on] = p
    out = {"env": a.env, "dtype": "float64", "envs": a.envs, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    for on, name in ((False, "policy_off"), (True, "policy_on")):
        out[name] = {"ms_per_env_step_median": statistics.median(ms[on]), "spread_ms": max(ms[on]) - min(ms[on]), "samples_ms": [round(v, 3) for v in ms[on]],
                     "pressure_iterations_per_solve": its[on], "piso_steps": piso[on],
                     "multilevel_cg_solves": envs[on]._domain.config_dump()["multilevel_cg_solves"]}
    out["gate_on_below_off_by_more_than_off_spread"] = bool(out["policy_off"]["ms_per_env_step_median"] - out["policy_on"]["ms_per_env_step_median"] > out["policy_off"]["spread_ms"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    for e in envs.values():
        e.close()


if __name__ == "__main__":
    main()
