"""The Lagrange-basis routes (DESIGN.md sections 4.18 and 5.0o) on one device, one process, warmed, the routes of a comparison
alternated, KZG_PERF_REPS repetitions each (default 3) with their min-max:
  (a) kzg_lagrange_prepare at 2^12, 2^16, 2^20 over an SRS of 2^20 points (each repetition replaces a basis of another size,
      so it builds), and the device memory the table adds (W x n x 128 bytes);
  (b) commitments per second with every slot in flight at 2^20 on resident inputs: kzg_commit_lagrange_submit against
      kzg_commit_evaluations_submit and kzg_commit_submit;
  (c) synchronous kzg_open_lagrange against kzg_open_evaluations at 2^12 and 2^20 (host arrays, wall time per call).
A route is called faster only where the difference of the medians exceeds the min-max spread of the older route.
`--kernels`: only a few openings at 2^20, for a separate `rocprofv3 --kernel-trace --stats` run (d).
GPU.  Writes JSON lines to profiles/r19_lagrange.jsonl (or the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "3")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG_N", "20"))
ROUNDS = int(os.environ.get("KZG_PERF_ROUNDS", "6"))  # jobs per slot in one repetition of (b)
SECRET = bytes(range(32))
R = K.R_MODULUS


def stats(ts, scale=1e3, unit="ms"):
    return {"median_" + unit: round(scale * float(np.median(ts)), 4), "min_" + unit: round(scale * min(ts), 4),
            "max_" + unit: round(scale * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def values(rng, n):
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
    return a


def verdict(new, old, unit, higher_is_better=False):
    """the newer route is faster only where the medians differ by more than the older route's own min-max spread"""
    spread = old["max_" + unit] - old["min_" + unit]
    diff = new["median_" + unit] - old["median_" + unit]
    gain = diff if higher_is_better else -diff
    return {"difference": round(diff, 4), "older_spread": round(spread, 4), "newer_is_faster": bool(gain > spread),
            "newer_is_slower": bool(-gain > spread)}


def pipelined_rate(eng, submit, bufs, n):
    """commitments per second with every slot in flight: ROUNDS jobs per slot"""
    slots = len(bufs)

    def run():
        for i in range(slots):
            submit(i, bufs[i], n)
        for _ in range(ROUNDS - 1):
            for i in range(slots):
                eng.wait(i)
                submit(i, bufs[i], n)
        for i in range(slots):
            eng.wait(i)

    return run, slots * ROUNDS


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "r19_lagrange.jsonl")
    n = 1 << LOG_N
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    rng = np.random.default_rng(19)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    try:
        host = values(rng, n)
        z = K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R)
        if kernels_only:
            eng.lagrange_prepare(LOG_N)
            y = eng.evaluate_evaluations_batch(host, [z])[0]
            for _ in range(4):
                eng.open_lagrange_limbs(host, z, y)
            return
        # ---- (a) the basis
        levels = eng.msm_config()["table_levels"]
        eng.lagrange_prepare(LOG_N)  # warm: the split twiddles of the largest size, the kernels
        for k in (12, 16, LOG_N):
            ts = []
            for _ in range(REPS):
                eng.lagrange_prepare(0)
                ts.append(timed(lambda: eng.lagrange_prepare(k)))
            emit({"what": "lagrange_prepare", "measured": True, "log_n": k, "srs_log_n": LOG_N, "reps": REPS, "build": stats(ts),
                  "table_levels": int(levels), "table_bytes": int(levels) * (1 << k) * 128})
        # ---- (c) synchronous openings, 2^12 then 2^LOG_N (one basis is held at a time)
        for k in (12, LOG_N):
            m = 1 << k
            ev = np.ascontiguousarray(host[:m])
            eng.lagrange_prepare(k)
            y = eng.evaluate_evaluations_batch(ev, [z])[0]
            new = lambda: eng.open_lagrange_limbs(ev, z, y)
            old = lambda: eng.open_evaluations_limbs(ev, z, y)
            assert new().compress() == old().compress()
            new(), old()
            tn, to = [], []
            for _ in range(REPS):
                to.append(timed(old))
                tn.append(timed(new))
            a, b = stats(tn), stats(to)
            emit({"what": "open_sync", "measured": True, "log_n": k, "reps": REPS, "kzg_open_lagrange": a, "kzg_open_evaluations": b,
                  "lagrange_vs_evaluations": verdict(a, b, "ms")})
        # ---- (b) commitments with every slot in flight at 2^LOG_N
        slots = eng.num_slots()
        bufs = [eng.dev_alloc(n * 32) for _ in range(slots)]
        try:
            for b in bufs:
                eng.dev_upload(b, host)
            routes = {"kzg_commit_lagrange_submit": eng.commit_lagrange_submit,
                      "kzg_commit_evaluations_submit": eng.commit_evaluations_submit, "kzg_commit_submit": eng.commit_submit}
            runs = {name: pipelined_rate(eng, fn, bufs, n) for name, fn in routes.items()}
            for run, _ in runs.values():
                run()  # warm
            rates = {name: [] for name in routes}
            for _ in range(REPS):
                for name, (run, jobs) in runs.items():
                    rates[name].append(jobs / timed(run))
            st = {name: stats(v, 1.0, "per_s") for name, v in rates.items()}
            emit({"what": "commit_pipelined", "measured": True, "log_n": LOG_N, "slots": slots, "jobs_per_repetition": slots * ROUNDS,
                  "reps": REPS, **st,
                  "lagrange_vs_evaluations": verdict(st["kzg_commit_lagrange_submit"], st["kzg_commit_evaluations_submit"], "per_s", True),
                  "lagrange_vs_commit": verdict(st["kzg_commit_lagrange_submit"], st["kzg_commit_submit"], "per_s", True),
                  "lagrange_over_commit": round(st["kzg_commit_lagrange_submit"]["median_per_s"] / st["kzg_commit_submit"]["median_per_s"], 4),
                  "evaluations_over_commit": round(st["kzg_commit_evaluations_submit"]["median_per_s"] / st["kzg_commit_submit"]["median_per_s"], 4)})
        finally:
            for b in bufs:
                eng.dev_free(b)
    finally:
        eng.close()
    with open(out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
