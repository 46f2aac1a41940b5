"""Multilinear openings at l = 20 and 16 on resident values: the whole chain of the four device rounds
(kzg_ml_fold_device, kzg_ml_commit_folds_device, kzg_ml_evaluations_device, kzg_ml_open_device) and each round, host wall time per
call; the streaming rounds with their algorithmic bytes per second; and the same proof by the route a caller had before these calls
-- the folds on the host with 16 threads (tests/host/ml_fold_cpu.cpp, built here with g++), one kzg_commit per level, kzg_open_sets
on the padded stack from host memory.  Every figure is a median of KZG_PERF_REPS >= 3 warmed repetitions with its min and max; the
two routes alternate.  KZG_PERF_ROUNDS_ONLY=1 runs the device rounds alone (for a kernel trace of the run).
GPU.  Writes JSON lines to profiles/r31_multilinear.jsonl (or the path given) and prints them."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "5")), 3)
ELLS = [int(x) for x in os.environ.get("KZG_PERF_ELLS", "20,16").split(",")]
ROUNDS_ONLY = os.environ.get("KZG_PERF_ROUNDS_ONLY", "0") == "1"
SECRET = bytes(range(32))
R = K.R_MODULUS
HBM_STREAM_GBS = 6290.0  # measured float4 copy on this part (8 TB/s is the specification)


def stats(ts):
    return {"median_ms": round(1e3 * float(np.median(ts)), 4), "min_ms": round(1e3 * min(ts), 4), "max_ms": round(1e3 * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def scalar(seed):
    return K.Scalar(int(np.random.default_rng(seed).integers(1, 1 << 62)) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % R)


def cpu_fold_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mlperf"), "libmlfold.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-pthread", "-o", out, os.path.join(ROOT, "tests", "host", "ml_fold_cpu.cpp")],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.ml_fold_cpu.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.ml_fold_cpu.restype = None
    return lib


def gbs(nbytes, st):
    return round(nbytes / (st["median_ms"] * 1e-3) / 1e9, 1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r31_multilinear.jsonl")
    eng = K.SetupArtifactsGenerator(SECRET).take(1 << max(ELLS))
    cpu = None if ROUNDS_ONLY else cpu_fold_lib()
    lines = []
    for ell in ELLS:
        n = 1 << ell
        rng = np.random.default_rng(ell)
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
        us, r, gamma = [scalar(100 + i) for i in range(ell)], scalar(7), scalar(8)
        d_evals, d_pyr = eng.dev_alloc(32 * n), eng.dev_alloc(32 * n)
        eng.dev_upload(d_evals, a)
        rounds = {
            "fold": lambda: eng.ml_fold_device(d_evals, ell, us, d_pyr),
            "commit_folds": lambda: eng.ml_commit_folds_device(d_pyr, ell),
            "evaluations": lambda: eng.ml_evaluations_device(d_evals, d_pyr, ell, r),
            "open": lambda: eng.ml_open_device(d_evals, d_pyr, ell, r, gamma),
        }

        def chain():
            return [fn() for fn in rounds.values()]

        proof = chain()  # warm: workspaces grown, kernels loaded
        chain()
        if ROUNDS_ONLY:
            for _ in range(REPS):
                chain()
            eng.dev_free(d_evals)
            eng.dev_free(d_pyr)
            continue
        us_rows = np.ascontiguousarray(np.stack([u.limbs() for u in us]), dtype=np.uint64)
        pyr = np.zeros((n, 4), dtype=np.uint64)

        def parent_route():
            t = {}
            t["fold_cpu16"] = timed(lambda: cpu.ml_fold_cpu(a.ctypes.data, ell, us_rows.ctypes.data, pyr.ctypes.data, 16))
            levels, at = [], 0
            for i in range(1, ell + 1):
                levels.append(pyr[at:at + (n >> i)])
                at += n >> i
            res = {}
            t["commit_per_level"] = timed(lambda: res.setdefault("folds", [eng.commit_limbs(lv) for lv in levels[:-1]]))
            stack = np.zeros((ell, n, 4), dtype=np.uint64)
            stack[0] = a
            for i, lv in enumerate(levels[:-1]):
                stack[i + 1, :len(lv)] = lv
            sets = [[r, K.Scalar(-r.v % R), K.Scalar(r.v * r.v % R)]]
            t["open_sets_host"] = timed(lambda: res.setdefault("open", eng.open_sets_limbs(stack, [0] * ell, sets, gamma)))
            t["total"] = t["fold_cpu16"] + t["commit_per_level"] + t["open_sets_host"]
            return t, res

        _, res = parent_route()  # warm, and the two routes give the same proof
        assert res["folds"] == proof[1] and res["open"][1] == proof[3]
        assert [[y.v for y in row] for row in res["open"][0]] == [[y.v for y in row] for row in proof[2]]
        new_total, new_rounds, old = [], {k: [] for k in rounds}, {}
        for _ in range(REPS):  # alternated
            new_total.append(timed(chain))
            for k, fn in rounds.items():
                new_rounds[k].append(timed(fn))
            t, _ = parent_route()
            for k, v in t.items():
                old.setdefault(k, []).append(v)
        st_new, st_old = stats(new_total), stats(old["total"])
        st_rounds = {k: stats(v) for k, v in new_rounds.items()}
        line = {"what": "ml_open_chain", "ell": ell, "reps": REPS, "chain_of_four_rounds": st_new, "rounds": st_rounds,
                "parent_route_total": st_old, "parent_route_parts": {k: stats(v) for k, v in old.items() if k != "total"},
                "parent_over_new": round(st_old["median_ms"] / st_new["median_ms"], 2),
                # algorithmic traffic of the streaming rounds (host wall time of the round: launch and wait included)
                "fold_bytes": 32 * (2 * n - 1), "fold_gbs": gbs(32 * (2 * n - 1), st_rounds["fold"]),
                "evaluations_bytes": 32 * (2 * n - 2), "evaluations_gbs": gbs(32 * (2 * n - 2), st_rounds["evaluations"]),
                "hbm_streaming_gbs_reference": HBM_STREAM_GBS}
        lines.append(line)
        print(json.dumps(line), flush=True)
        eng.dev_free(d_evals)
        eng.dev_free(d_pyr)
    eng.close()
    if lines:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
