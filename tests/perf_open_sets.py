"""Openings at several point sets at n = 2^20 on resident inputs, PLONK's shape: nine polynomials at z,
one at z w, proved
  * route A, the way without kzg_open_sets, in the same process: kzg_open_combined_submit of the nine in one slot and
    kzg_open_submit of the tenth in another, both in flight, both waited -- two MSMs, two G1 elements;
  * route B: kzg_open_sets_submit + kzg_wait_sets -- one MSM, one G1 element.
Both are warmed, then alternated A, B, A, B, ... for KZG_PERF_REPS repetitions (default 9): host wall time per call, the median
and the min-max of each.  The claim checked: B is faster than A by more than A's own min-max spread in that run.  Then B's
split with kzg_set_timing (the passes from kzg_get_combine_ms; the scans and the MSM from kzg_get_times), and B alone on a
three-set shape: sixteen polynomials over {z}, {z, z w}, {z, z w, z / w}.
GPU.  Writes JSON lines to profiles/r15_open_sets.jsonl (or the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "9")), 9)
LOG_N = int(os.environ.get("KZG_PERF_LOG_N", "20"))
SECRET = bytes(range(32))
R = K.R_MODULUS


def stats(ts):
    return {"median_ms": round(1e3 * float(np.median(ts)), 4), "min_ms": round(1e3 * min(ts), 4), "max_ms": round(1e3 * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def split_of(eng, fn, reps):
    """medians of the passes, the scans and the MSM of route B, from the events of timed jobs"""
    eng.set_timing(True)
    passes, scans, msm = [], [], []
    for _ in range(reps + 1):
        fn()
        tm = eng.times(0)
        passes.append(eng.combine_ms(0))
        scans.append(tm["quotient_ms"])
        msm.append(tm["total_ms"] - tm["quotient_ms"])
    eng.set_timing(False)
    return {"passes_ms": round(float(np.median(passes[1:])), 4), "scans_ms": round(float(np.median(scans[1:])), 4),
            "msm_ms": round(float(np.median(msm[1:])), 4)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_open_sets.jsonl")
    n = 1 << LOG_N
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    rng = np.random.default_rng(15)
    tmax = 16
    host = rng.integers(0, 1 << 64, size=(tmax, n, 4), dtype=np.uint64)
    host[..., 3] = rng.integers(0, R >> 192, size=(tmax, n), dtype=np.uint64)
    w = K.domain_root(LOG_N).v
    zv = int(rng.integers(1, 1 << 62)) ** 4 % R
    z, zw, zwi = K.Scalar(zv), K.Scalar(zv * w % R), K.Scalar(zv * pow(w, -1, R) % R)
    gamma = K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R)
    dptr = eng.dev_alloc(tmax * n * 32)
    lines = []
    try:
        eng.dev_upload(dptr, host)
        # ---- PLONK's shape
        t, set_of, sets = 10, [0] * 9 + [1], [[z], [zw]]
        state = {}

        def route_b():
            eng.open_sets_submit(0, dptr, n, t, set_of, sets, gamma)
            state["ys"], state["pi"] = eng.wait_sets(0, set_of, sets)

        route_b()
        y_last = state["ys"][9][0]

        def route_a():
            eng.open_combined_submit(0, dptr, n, 9, z, gamma)
            eng.open_submit(1, dptr + 9 * n * 32, n, zw, y_last)
            state["a"] = (eng.wait_combined(0, 9), eng.wait(1))

        route_a()
        route_b()
        # the same values by both routes
        assert [y.v for y in state["a"][0][0]] == [row[0].v for row in state["ys"][:9]]
        ta, tb = [], []
        for _ in range(REPS):
            ta.append(timed(route_a))
            tb.append(timed(route_b))
        a, b = stats(ta), stats(tb)
        spread_a = a["max_ms"] - a["min_ms"]
        line = {"what": "open_sets_plonk_shape", "log_n": LOG_N, "t": t, "sets": "{z} x 9, {z w} x 1", "reps": REPS,
                "route_a_combined_plus_open": a, "route_b_open_sets": b,
                "a_over_b": round(a["median_ms"] / b["median_ms"], 3),
                "a_minus_b_ms": round(a["median_ms"] - b["median_ms"], 4), "a_spread_ms": round(spread_a, 4),
                "b_faster_by_more_than_a_spread": bool(a["median_ms"] - b["median_ms"] > spread_a),
                "proof_elements": {"a": 2, "b": 1}}
        line["route_b_split"] = split_of(eng, route_b, REPS)
        lines.append(line)
        print(json.dumps(line), flush=True)
        # ---- three sets, B only
        t3, set_of3, sets3 = 16, [0] * 8 + [1] * 5 + [2] * 3, [[z], [z, zw], [z, zw, zwi]]

        def route_b3():
            eng.open_sets_submit(0, dptr, n, t3, set_of3, sets3, gamma)
            eng.wait_sets(0, set_of3, sets3)

        route_b3()
        route_b3()
        line = {"what": "open_sets_three_sets", "log_n": LOG_N, "t": t3, "sets": "{z} x 8, {z, z w} x 5, {z, z w, z / w} x 3",
                "reps": REPS, "route_b_open_sets": stats([timed(route_b3) for _ in range(REPS)])}
        line["route_b_split"] = split_of(eng, route_b3, REPS)
        lines.append(line)
        print(json.dumps(line), flush=True)
    finally:
        eng.dev_free(dptr)
        eng.close()
    with open(out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
