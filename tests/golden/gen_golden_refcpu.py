"""Records what the reference's own CPU functions (oracle/_ref/libatom_ref.so, built by oracle/Makefile from the reference source)
return for the inputs of the tests that use them, into tests/golden/ref_cpu_calls.npz; tests/ref_golden.py replays those results
where the library is not built.  Needs the library; the GPU modules need a GPU as well (their inputs come from the device).

    python tests/golden/gen_golden_refcpu.py            # the CPU tests (tests/test_oracle_ref.py)
    python tests/golden/gen_golden_refcpu.py --gpu      # + tests/test_gpu_ref.py and the reference test of tests/test_gpu_kv.py

Recordings are added to the file (a call already recorded is checked against the library, not duplicated)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ref_cpu_calls.npz"))
    args = ap.parse_args()
    from tests import ref_golden as R
    if not R.lib_built():
        raise SystemExit("oracle/_ref/libatom_ref.so is not built: make -C oracle where the reference source is present")
    targets = ["tests/test_oracle_ref.py"]
    if args.gpu:
        targets += ["tests/test_gpu_ref.py", "tests/test_gpu_kv.py::test_append_and_decode_vs_reference_cpu_implementation"]
    env = dict(os.environ, ATOM_REF_RECORD=os.path.abspath(args.out))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *targets]
                       + ([] if args.gpu else ["-m", "not gpu"]), cwd=ROOT, env=env)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
