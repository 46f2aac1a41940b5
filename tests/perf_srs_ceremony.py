"""Powers-of-tau ceremonies at n = 4096, 2^16 and 2^20 SRS points (KZG_PERF_NS overrides):
  * kzg_srs_update beside kzg_srs_generate_g1 at the same n -- the other way this library has of producing the tables of a
    setup -- as medians of KZG_PERF_REPS calls (default 7) alternated call by call, and the update split into ladder kernel,
    normalisation, table rebuild and slot setup;
  * kzg_srs_verify as a median, and split into subgroup check, the two MSMs and the host pairing;
  * the host route as an extrapolation: the C oracle's time for one scalar multiplication of a G1 point on one core, times n.
The splits come from the library's own phase clock (KZG_SRS_TRACE=1: host clock around work that ends in a device
synchronise, one line on stderr per call), taken in calls of their own: a traced update waits for the device after every phase.
GPU.  Writes JSON lines to profiles/r13_srs_ceremony.jsonl (or the path given) and prints them."""
import json
import os
import random
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes as O  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "7"))
NS = [int(x) for x in os.environ.get("KZG_PERF_NS", "4096,65536,1048576").split(",") if x]
SECRET = bytes(range(32))
TAU = bytes(range(100, 132))
R = K.R_MODULUS


def traced(fn):
    """runs fn with the phase clock on; returns {phase: ms} of the line it printed"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["KZG_SRS_TRACE"] = "1"
        try:
            fn()
        finally:
            os.environ.pop("KZG_SRS_TRACE")
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    return {k: float(v) for k, v in re.findall(r"(\w+)_ms=([0-9.]+)", text)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_srs_ceremony.jsonl")
    recs = []

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    g2 = np.stack([K.srs_g2_at(SECRET, i) for i in range(2)])
    # the host route: one scalar multiplication of a point that is not the generator, full-width scalars, one core
    rnd = random.Random(3)
    pt = O.p1_mult(O.p1_generator(), rnd.randrange(1, R))
    ks = [rnd.randrange(R) for _ in range(200)]
    O.p1_mult(pt, ks[0])
    t0 = time.perf_counter()
    for k in ks:
        O.p1_mult(pt, k)
    host_us = 1e6 * (time.perf_counter() - t0) / len(ks)
    eng = K.Engine(0)
    try:
        for n in NS:
            eng.srs_generate(SECRET, n)
            eng.srs_update(TAU)  # warm-up of every kernel at this shape
            assert eng.srs_verify(np.stack([g2[0], K.g2_mul(g2[1], TAU)])) == (True, K.KZG_SRS_OK, None)
            gen, upd, ver = [], [], []
            for _ in range(REPS):
                gen.append(timed(lambda: eng.srs_generate(SECRET, n)))
                upd.append(timed(lambda: eng.srs_update(TAU)))
                g2u = np.stack([g2[0], K.g2_mul(g2[1], TAU)])
                res = []
                ver.append(timed(lambda: res.append(eng.srs_verify(g2u))))
                assert res[0] == (True, K.KZG_SRS_OK, None)
            split_u = traced(lambda: eng.srs_update(TAU))
            split_v = traced(lambda: eng.srs_verify(g2, require_generator=False))  # (rejected at the pairing: the same work)
            cfg = eng.msm_config()
            emit({"what": "srs_update", "n": n, "reps": REPS, "table_levels": cfg["table_levels"],
                  "srs_generate_ms": round(1e3 * float(np.median(gen)), 3), "srs_update_ms": round(1e3 * float(np.median(upd)), 3),
                  "srs_update_min_ms": round(1e3 * min(upd), 3), "srs_update_max_ms": round(1e3 * max(upd), 3),
                  "traced_call": {k + "_ms": v for k, v in split_u.items()}})
            emit({"what": "srs_verify", "n": n, "reps": REPS, "srs_verify_ms": round(1e3 * float(np.median(ver)), 3),
                  "srs_verify_min_ms": round(1e3 * min(ver), 3), "srs_verify_max_ms": round(1e3 * max(ver), 3),
                  "traced_call": {k + "_ms": v for k, v in split_v.items()}})
            emit({"what": "host_route_extrapolated", "n": n, "oracle_scalar_mult_us": round(host_us, 1),
                  "extrapolated_one_core_ms": round(host_us * n / 1e3, 1),
                  "note": "the C oracle's per-point time on one core times n; not a run of n points"})
    finally:
        eng.close()
        with open(out, "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
