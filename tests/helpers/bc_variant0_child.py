"""Child process of tests/test_gpu_baseconv_edges.py::test_runtime_m_kernels_for_small_bases: started with FHE_BC_VARIANT=0 in its
environment (the library reads the switch once, at its first conversion), it runs the exact conversion on the parent's inputs and
prints one JSON line {case: SHA-256 of the output words}."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    assert os.environ.get("FHE_BC_VARIANT") == "0"
    import fhe_reliability_gpu_amd as F
    from helpers import bc_edge_cases as E

    eng = F.default_engine()
    out = {}
    for m in E.VARIANT0_SIZES:
        for big in (False, True):
            mi, mo, x, _, _ = E.small_case(F, m, E.VARIANT0_K, big)
            out[f"m{m}-{'u64' if big else 'f64'}"] = E.sha(E.convert(F, eng, mi, mo, x))
    mi, mo, x, _, _, cols = E.long_case(F)
    out["long"] = E.sha(E.convert(F, eng, mi, mo, x)[:, cols])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
