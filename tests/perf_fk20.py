"""FK20 (kzg_cells_and_proofs_fk20) against kzg_cells_and_proofs, one polynomial per call for the latter.  The SRS has exactly
n points and max_batch is 128 for the baseline.  Reports polynomials/s of both, the batch at which FK20 overtakes the cells
call, and the cost of kzg_fk20_prepare.  GPU; writes JSON lines to profiles/r07_fk20.jsonl (or the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes as O  # noqa: E402  (bench inputs only)

REPS = int(os.environ.get("KZG_PERF_REPS", "5"))


def median_time(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def polys(n, batch):
    base = np.ascontiguousarray(O.bench_coefficients(n), dtype=np.uint64).reshape(n, 4)
    out = np.repeat(base[None], batch, axis=0)
    out[:, 0, 0] = np.arange(batch, dtype=np.uint64) + 1  # distinct polynomials
    return out


def shape(n, log_n, log_l, batches, baseline=True):
    eng = K.SetupArtifactsGenerator(bytes(range(32))).take(n)
    eng.set_max_batch(128)
    t0 = time.perf_counter()
    eng.fk20_prepare(n, log_l)
    prep = time.perf_counter() - t0
    recs = []
    t_cells = None
    if baseline:
        c = polys(n, 1)[0]
        t_cells = median_time(lambda: eng.cells_and_proofs_limbs(c, log_n, log_l), REPS)
    for b in batches:
        c = polys(n, b)
        t = median_time(lambda: eng.cells_and_proofs_fk20(c, log_n, log_l, cells=False), REPS)
        rec = {"n": n, "N": 1 << log_n, "l": 1 << log_l, "batch": b, "fk20_ms": round(1e3 * t, 3),
               "fk20_polys_per_s": round(b / t, 1), "prepare_ms": round(1e3 * prep, 1)}
        if t_cells is not None:
            rec.update({"cells_ms": round(1e3 * t_cells, 3), "cells_polys_per_s": round(1 / t_cells, 1),
                        "speedup": round(b * t_cells / t, 2)})
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    eng.close()
    return recs


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_fk20.jsonl")
    cases = [(4096, 13, 6, [64, 1, 2, 4, 8, 16, 32], True), (4096, 12, 0, [1], True), (1 << 16, 17, 6, [1], False)]
    with open(out, "w") as f:
        for n, log_n, log_l, batches, base in cases:
            for rec in shape(n, log_n, log_l, batches, base):
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
