"""Outputs of the resident sweep k_sweep_r8 in both instantiations (VMC sweeps, then DMC steps) on the headline (H2O)8 system, for a
byte-for-byte comparison of two builds of the library (PQA_LIB selects the build).  bench.py --mode dmc runs the periodic C5 system,
which never reaches k_sweep_r8: this covers k_sweep_r8<true, ...>.
usage: python tools/r8_ab_outputs.py dump OUT.npz [--walkers 4096]    (PQA_LIB=... for the other build)
       python tools/r8_ab_outputs.py cmp A.npz B.npz                  (exit status 1 unless every array is bitwise equal)"""
import argparse, os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["dump", "cmp"])
ap.add_argument("files", nargs="+")
ap.add_argument("--walkers", type=int, default=4096)
args = ap.parse_args()

if args.what == "cmp":
    a, b = np.load(args.files[0]), np.load(args.files[1])
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].tobytes() != b[k].tobytes()]
    for k in sorted(a.files):
        print(f"{k:8s} {a[k].shape} {'DIFFERS' if k in bad else 'identical'}")
    print("bitwise identical" if not bad else f"differ: {bad}")
    sys.exit(1 if bad else 0)

os.environ["PQA_R8"] = "1"  # the resident sweep k_sweep_r8 at any walker count (read when the handle is created)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyqmc_amd as pa

W = args.walkers
mol = pa.systems.water_cluster(); mf = pa.systems.random_mf(mol)
wf = pa.generate_wf(mol, mf); dev = wf.fused_device()
wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(11)))
acc, en, rec = dev.vmc_sweeps(0.3, 2, seed=21, energy=True, record=True)
out = {"vmc_acc": np.asarray(acc), "vmc_en": np.asarray(en), "vmc_rec": np.asarray(rec), "vmc_x": dev.configs()}
sign, logv = dev.value()
out.update(vmc_sign=np.asarray(sign), vmc_logv=np.asarray(logv))
w = np.ones(W)
et = float(np.real(en[-1][5]))
avg, dacc = dev.dmc_steps(0.02, 3, w, 10.0, et, et, seed=5)
sign, logv = dev.value()
out.update(dmc_avg=avg, dmc_acc=dacc, dmc_w=w, dmc_x=dev.configs(), dmc_sign=np.asarray(sign), dmc_logv=np.asarray(logv))
np.savez(args.files[0], **out)
print(f"[r8_ab_outputs] {W} walkers, {len(out)} arrays -> {args.files[0]}")
