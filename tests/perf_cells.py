"""Cells of a domain and their multiproofs (kzg_cells_and_proofs) against the per-cell paths they replace: kzg_open_points_submit
(l > 1) or kzg_open_submit (l = 1) with the coefficients on the device and every slot in flight.  The SRS has exactly n
points and max_batch is 128.  GPU; writes JSON lines to profiles/r06_cells.jsonl (or the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cells_oracle as CO  # noqa: E402
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes as O  # noqa: E402  (bench inputs only)

REPS = int(os.environ.get("KZG_PERF_REPS", "10"))


def pipelined(eng, submits):
    """every submit through the slots, the oldest collected when all are busy; returns seconds"""
    slots = eng.num_slots()
    t0 = time.perf_counter()
    inflight = []
    for i, submit in enumerate(submits):
        s = i % slots
        if len(inflight) == slots:
            eng.wait(inflight.pop(0))
        submit(s)
        inflight.append(s)
    while inflight:
        eng.wait(inflight.pop(0))
    return time.perf_counter() - t0


def median_time(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def shape(n, log_n, log_l, compare):
    eng = K.SetupArtifactsGenerator(bytes(range(32))).take(n)
    eng.set_max_batch(128)
    c = O.bench_coefficients(n)
    ncell = (1 << log_n) >> log_l
    t_call = median_time(lambda: eng.cells_and_proofs_limbs(c, log_n, log_l), REPS)
    rec = {"n": n, "N": 1 << log_n, "l": 1 << log_l, "cells": ncell, "call_ms": round(1e3 * t_call, 3),
           "blobs_per_s": round(1 / t_call, 2), "proofs_per_s": round(ncell / t_call, 1)}
    if compare:
        d = eng.dev_alloc(n * 32)
        eng.dev_upload(d, np.ascontiguousarray(c))
        cells, proofs = eng.cells_and_proofs_limbs(c, log_n, log_l)
        if log_l == 0:
            pts = [(K.Scalar(CO.cell_points(log_n, 0, j)[0]), K.Scalar.from_limbs(cells[j])) for j in range(ncell)]
            submits = [lambda s, z=z, y=y: eng.open_submit(s, d, n, z, y) for z, y in pts]
        else:
            l = 1 << log_l
            cl = [([K.Scalar(z) for z in CO.cell_points(log_n, log_l, j)],
                   [K.Scalar.from_limbs(v) for v in cells[j * l:(j + 1) * l]]) for j in range(ncell)]
            submits = [lambda s, zs=zs, ys=ys: eng.open_points_submit(s, d, n, zs, ys) for zs, ys in cl]
        pipelined(eng, submits[: eng.num_slots() * 2])  # warm
        t_base = float(np.median([pipelined(eng, submits) for _ in range(max(REPS // 3, 1))]))
        rec.update({"baseline": "kzg_open_submit" if log_l == 0 else "kzg_open_points_submit",
                    "baseline_ms": round(1e3 * t_base, 3), "baseline_proofs_per_s": round(ncell / t_base, 1),
                    "speedup": round(t_base / t_call, 2)})
        eng.dev_free(d)
    eng.close()
    return rec


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_cells.jsonl")
    cases = [(4096, 13, 6, True), (4096, 12, 0, True), (4096, 13, 4, False), (1 << 16, 17, 6, False)]
    with open(out, "w") as f:
        for n, log_n, log_l, compare in cases:
            rec = shape(n, log_n, log_l, compare)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
