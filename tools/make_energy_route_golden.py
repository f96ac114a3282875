"""Fixture energy_routes_parent: the outputs of every case of tests/test_gpu_energy_route.py from the library of the commit BEFORE the
energy pass got its plan.  Needs the GPU and that commit's library:

    PQA_LIB=<parent worktree>/pyqmc_amd/lib/libpyqmc_amd.so python tools/make_energy_route_golden.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_energy_route as routes  # noqa: E402

assert os.environ.get("PQA_LIB"), "point PQA_LIB at the parent commit's library"
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "energy_routes_parent.npz")
arrays = routes.record(out)
print(f"wrote {out}: {len(routes.CASES)} cases, {len(arrays)} arrays, {os.path.getsize(out)} bytes")
