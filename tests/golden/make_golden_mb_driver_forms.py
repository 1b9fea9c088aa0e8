"""Writes tests/golden/mb_driver_forms.npz, the fixture of tests/test_gpu_mb_driver_forms.py: what every step of every case of that
module leaves behind, to the bit.  Needs the GPU; run from the repository root (``python tests/golden/make_golden_mb_driver_forms.py``)
with the library built from the commit whose bits are the yardstick.  Not run by the suite.

Every case is run twice on fresh domains and must repeat itself bit for bit, and must show the condition it is in the fixture for
(``shows_its_condition``): a case that does not is to get another state, not another condition."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_gpu_mb_driver_forms as T  # noqa: E402


def main(path, only=None):
    out, bad = {}, []
    for name in T.CASES:
        if only and not any(name.startswith(o) for o in only):
            continue
        a, b = (T.run_case(name, None, None, None, os.environ.__setitem__, lambda k: os.environ.pop(k, None))[0] for _ in range(2))
        for f in T.FIELDS:
            assert np.array_equal(a[f], b[f]), (name, f, "a case did not repeat its bits")
            out[f"{name}.{f}"] = a[f]
        ok = bool(T.shows_its_condition(name, a))
        if not ok:
            bad.append(name)
        print(name, "its", a["its"].tolist(), "status", a["status"].tolist(), "env_status", a["env_status"].tolist(), "jacobi", a["jacobi"].tolist(),
              "ladder", a["ladder"].tolist(), "trial", a["trial"].tolist(), "hints[32:48]", a["hints"][:, 32:].tolist(),
              "pressure0 mean/max/systems", [(float(c[8:9].view(np.float64)[0]), int(c[9]), int(c[10])) for c in a["counters"]],
              "->", "ok" if ok else "CONDITION NOT SHOWN", flush=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20
    assert not bad, f"cases that do not show their condition: {bad}"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN, sys.argv[2:])
