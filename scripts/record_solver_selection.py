"""Record what the selection of the (A A')^-1 solver does with every case of
tests/selection_cases.py under every combination of its options:

    python scripts/record_solver_selection.py OUT.json [case ...]

Per (case, options): the name of the solver ``projections`` chose, whether the projector carries
a row permutation, whether ``_banded_row_order`` returned one, and the increases of
``ipx_launch_count()`` / ``ipx_read_count()`` across the fresh ``projections(A)`` call.
tests/golden/solver_selection.json is this script's output at the commit before the selection
was rewritten as a rule list; tests/test_gpu_solver_selection.py calls ``measure`` and compares.
Needs a GPU.  Uses no name of the library younger than that commit.
"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ip-nonlinear-solver_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def measure(A, max_rows, options):
    """One entry of the table for the host matrix A: uploaded anew, so every per-pattern cache
    is cold."""
    import numpy as np
    from ipsolver import _hip, device as dv, projector as proj
    from ipsolver.dense import DenseNormalSolver
    lib = _hip.load()
    policy, border, link = options
    keep = DenseNormalSolver.MAX_ROWS_FROM_SPARSE
    if max_rows is not None:
        DenseNormalSolver.MAX_ROWS_FROM_SPARSE = max_rows
    try:
        with proj.wide_band(policy), proj.border_columns(border), proj.link_rows(link), \
                warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Ad = proj.as_device_matrix(A)
            proj._last_solver[0] = None
            launches, reads = int(lib.ipx_launch_count()), int(lib.ipx_read_count())
            try:
                Z = proj.projections(Ad)[0]
                name = proj.last_normal_solver()
            except (NotImplementedError, np.linalg.LinAlgError) as exc:
                Z, name = None, "raises:" + type(exc).__name__
            launches = int(lib.ipx_launch_count()) - launches
            reads = int(lib.ipx_read_count()) - reads
            sparse = isinstance(Ad, dv.DeviceCSR)
            return {"solver": name,
                    "row_perm": getattr(getattr(Z, "projector", None), "row_perm", None) is not None,
                    "row_order": bool(sparse and proj._banded_row_order(Ad) is not None),
                    "launches": launches, "reads": reads}
    finally:
        DenseNormalSolver.MAX_ROWS_FROM_SPARSE = keep


def main(out, names):
    import selection_cases as sc
    table = {}
    for name in names or sorted(sc.CASES):
        A, max_rows = sc.build(name)
        table[name] = {"shape": list(A.shape), "max_rows": max_rows, "entries": {}}
        for options in sc.OPTIONS:
            table[name]["entries"][sc.option_id(options)] = measure(A, max_rows, options)
        print(name, A.shape, sorted({e["solver"] or "-" for e in table[name]["entries"].values()}),
              flush=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
