"""Writes tests/golden/sb_driver_forms.npz, the fixture of tests/test_gpu_sb_driver_forms.py: what every solve of every case of that
module returns, to the bit.  Needs the GPU; run from the repository root (``python tests/golden/make_golden_sb_driver_forms.py``) with
the library built from the commit whose bits are the yardstick.  Not run by the suite.

Every case is solved twice on fresh handles and must repeat itself bit for bit, and must show the condition it is in the fixture
for (``shows_its_condition``): a case that does not is to get other parameters, not another condition."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_gpu_sb_driver_forms as T  # noqa: E402


def main(path):
    out, bad = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name in T.CASES:
            a, b = (T.run_case(name, None, os.environ.__setitem__, lambda k: os.environ.pop(k, None), tmp) for _ in range(2))
            for f in T.FIELDS:
                assert np.array_equal(a[f], b[f]), (name, f, "a case did not repeat its bits")
                out[f"{name}.{f}"] = a[f]
            ok = bool(T.shows_its_condition(name, a))
            if not ok:
                bad.append(name)
            print(name, "used", a["used"].tolist(), "converged", a["conv"].tolist(), "status", a["status"].tolist(), "counts", a["counts"].tolist(),
                  "residual", ["%.3e" % v for v in a["res"].view(np.float64).ravel()], "->", "ok" if ok else "CONDITION NOT SHOWN", flush=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20
    assert not bad, f"cases that do not show their condition: {bad}"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN)
