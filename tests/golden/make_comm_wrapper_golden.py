"""The golden of tests/test_comm_wrappers_cpu.py.

comm_wrapper_calls.json holds, per case of tests/commrec.py, every call the
native multi-GPU wrappers of feddct_amd/comm.py made on the recorder standing
in for libfedagg_comm.so, with the attributes they left and the exception
text where they raised; and the ten classes' constructor signatures.  It was
recorded from commit 111fd7d, the last one whose five plan classes and five
aggregator classes each carried their own copy of the plumbing, NOT from the
module as it stands:

    mkdir /tmp/parent && git archive 111fd7d | tar -x -C /tmp/parent
    cp feddct_amd/*.so /tmp/parent/feddct_amd/     # or build there; csrc/ is the same
    python tests/golden/make_comm_wrapper_golden.py /tmp/parent

which imports the feddct_amd package of the tree named and runs this tree's
tests/commrec.py against its comm module."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "111fd7d"
OUT = os.path.join(HERE, "comm_wrapper_calls.json")


def dumps(x):
    """The one spelling both sides compare: True is not 1, a tuple is a list."""
    return json.dumps(x, sort_keys=True, separators=(",", ":"))


def record(tree):
    """{"signatures": ..., "cases": {name: record}} of the comm module of ``tree``."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import commrec
    for m in [m for m in sys.modules if m == "feddct_amd" or m.startswith("feddct_amd.")]:
        del sys.modules[m]
    sys.path.insert(0, tree)
    from feddct_amd import comm as C
    assert os.path.realpath(C.__file__) == os.path.realpath(
        os.path.join(tree, "feddct_amd", "comm.py")), C.__file__
    real = C._clib
    try:
        cases = commrec.record(C, lambda rec: setattr(C, "_clib", rec))
    finally:
        C._clib = real
    return {"signatures": commrec.signatures(C), "cases": cases}


def main(argv):
    got = record(os.path.realpath(argv[1]))
    with open(OUT, "w") as f:   # one case per line
        rows = ",\n".join(f"{json.dumps(k)}:{dumps(v)}" for k, v in got["cases"].items())
        f.write('{"parent":"%s","signatures":%s,"cases":{\n%s\n}}\n'
                % (PARENT, dumps(got["signatures"]), rows))
    print(len(got["cases"]), "cases ->", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
