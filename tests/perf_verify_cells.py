"""Batch verification of cells (kzg_verify_cells_batch) at the DAS shape (4096, 8192, 64) with 128 commitments and K = 128,
1 024 and 16 384 records (random cells of the 128 polynomials), against kzg_verify_points measured on a sample of single cells
and scaled to the same K over the host's cores.  GPU; writes JSON lines to profiles/r09_verify_cells.jsonl (or the path
given) and prints them.  KZG_PERF_ONLY_BATCH=1 times only the batch call (for a kernel trace)."""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bigint_twin as T  # noqa: E402
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import ntt_oracle as NO  # noqa: E402
import oracle_ctypes as O  # noqa: E402  (bench inputs only)

REPS = int(os.environ.get("KZG_PERF_REPS", "5"))
ONLY_BATCH = os.environ.get("KZG_PERF_ONLY_BATCH") == "1"
SECRET = bytes(range(32))


def median_time(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_verify_cells.jsonl")
    n, log_n, log_l, B = 4096, 13, 6, 128
    M, l = 1 << (log_n - log_l), 1 << log_l
    g2 = [K.srs_g2_at(SECRET, i) for i in range(l + 1)]
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    try:
        base = np.ascontiguousarray(O.bench_coefficients(n), dtype=np.uint64).reshape(n, 4)
        c = np.repeat(base[None], B, axis=0)
        c[:, 0, 0] = np.arange(B, dtype=np.uint64) + 1
        cells, proofs = eng.cells_and_proofs_fk20(c, log_n, log_l)
        coms = np.stack([eng.commit_limbs(c[b]).p1 for b in range(B)])
        vals = cells.reshape(B, M, l, 4)
        prf = np.stack([np.stack([p.p1 for p in proofs[b]]) for b in range(B)])
        # kzg_verify_points on a sample of single cells, one host thread each: scaled by the host's cores
        sample = 4
        g1 = np.stack([np.array(T.g1_to_blst_p1_limbs(p), dtype=np.uint64) for p in T.srs_g1(SECRET, l)])
        w = NO.domain_root(log_n)
        t_single = None
        if not ONLY_BATCH:
            t0 = time.perf_counter()
            for s in range(sample):
                b, j = s, 3 * s
                zs = [K.Scalar(pow(w, j + M * i, K.R_MODULUS)) for i in range(l)]
                ys = [K.Scalar(v) for v in K.limbs_to_scalars(vals[b, j])]
                assert K.verify_points(K.G1Point(coms[b]), K.G1Point(prf[b, j]), zs, ys, g1, g2)
            t_single = (time.perf_counter() - t0) / sample
        cores = min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16")))
        with open(out, "w") as f:
            for k in (128, 1024, 16384):
                rnd = random.Random(k)
                recs = [(rnd.randrange(B), rnd.randrange(M)) for _ in range(k)]
                idx = np.array([r[0] for r in recs], dtype=np.uint32)
                ids = np.array([r[1] for r in recs], dtype=np.uint32)
                rv = np.ascontiguousarray(vals[idx, ids])
                rp = np.ascontiguousarray(prf[idx, ids])
                assert eng.verify_cells_batch(coms, idx, ids, rv, rp, log_n, log_l, g2)
                t = median_time(lambda: eng.verify_cells_batch(coms, idx, ids, rv, rp, log_n, log_l, g2), REPS)
                rec = {"n": n, "N": 1 << log_n, "l": l, "commitments": B, "cells": k, "ms_per_call": round(1e3 * t, 3),
                       "cells_per_s": round(k / t, 1)}
                if t_single is not None:
                    rec.update({"verify_points_ms_per_cell_one_core": round(1e3 * t_single, 3), "host_cores": cores,
                                "verify_points_scaled_ms": round(1e3 * t_single * k / cores, 1),
                                "speedup_vs_verify_points_all_cores": round(t_single * k / cores / t, 1)})
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
