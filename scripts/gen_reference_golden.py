#!/usr/bin/env python3
"""Rewrites tests/golden/reference_outputs.npz: the outputs of the reference's own kernels (oracle/_ref, built by
`make -C oracle ref` where the reference's sources are present) for every call the CPU tests make through
tests/oracle_lib.reference().  Runs those tests with AH_RECORD_REFERENCE set, which makes reference() call the live
libraries and store each answer under a digest of the call's inputs; a machine without oracle/_ref then replays them.

    python scripts/gen_reference_golden.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import oracle_lib as OL  # noqa: E402

# the test modules that call OL.reference()
MODULES = ["tests/test_oracle_vs_reference.py", "tests/test_ddsum_host.py", "tests/test_sum_short.py"]


def main():
    if OL.load_reference() is None:
        sys.exit("oracle/_ref is not built (make -C oracle ref needs the reference's sources)")
    tmp = OL.REFERENCE_GOLDEN + ".tmp.npz"
    env = dict(os.environ, **{OL.RECORD_ENV: tmp})
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider"] + MODULES, cwd=ROOT, env=env)
    os.replace(tmp, OL.REFERENCE_GOLDEN)
    print(f"wrote {os.path.relpath(OL.REFERENCE_GOLDEN, ROOT)}: {os.path.getsize(OL.REFERENCE_GOLDEN)} bytes")


if __name__ == "__main__":
    main()
