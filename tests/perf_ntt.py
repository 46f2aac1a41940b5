"""NTT at 2^16, 2^20 and 2^22: time per direction of kzg_ntt_device (device buffers, synchronous call: host round trip
included, the kernels' own span is in a rocprofv3 kernel trace of this script), and commitments per second at 2^20 from
evaluations (kzg_commit_evaluations_submit) against kzg_commit_submit, every slot in flight.  GPU; prints JSON lines."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

R = K.R_MODULUS


def random_images(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    c[:, 3] %= np.uint64(R >> 192)
    return c


def pipelined(eng, submit, reps):
    slots = eng.num_slots()
    for phase in ("warm", "timed"):
        count = 10 if phase == "warm" else reps
        t0 = time.perf_counter()
        inflight = []
        for i in range(count):
            s = i % slots
            if len(inflight) == slots:
                eng.wait(inflight.pop(0))
            submit(s)
            inflight.append(s)
        while inflight:
            eng.wait(inflight.pop(0))
        dt = time.perf_counter() - t0
    return reps / dt


def main():
    reps = int(os.environ.get("KZG_PERF_REPS", "40"))
    n20 = 1 << 20
    eng = K.SetupArtifactsGenerator(bytes(range(32))).take(n20)
    for k in (16, 20, 22):
        n = 1 << k
        a = random_images(n, k)
        d_in, d_out = eng.dev_alloc(n * 32), eng.dev_alloc(n * 32)
        eng.dev_upload(d_in, a)
        row = {"log_n": k}
        for name, inv in (("forward_us", False), ("inverse_us", True)):
            for _ in range(3):
                eng.ntt_device(d_in, d_out, n, inv)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.ntt_device(d_in, d_out, n, inv)
                ts.append(time.perf_counter() - t0)
            row[name] = round(1e6 * float(np.median(ts)), 1)
        print(json.dumps(row), flush=True)
        eng.dev_free(d_in)
        eng.dev_free(d_out)
    e = random_images(n20, 1)
    d = eng.dev_alloc(n20 * 32)
    eng.dev_upload(d, e)
    commit_rate = pipelined(eng, lambda s: eng.commit_submit(s, d, n20), reps)
    evals_rate = pipelined(eng, lambda s: eng.commit_evaluations_submit(s, d, n20), reps)
    print(json.dumps({"log_n": 20, "commit_per_s": round(commit_rate, 1), "commit_evaluations_per_s": round(evals_rate, 1),
                      "ratio": round(evals_rate / commit_rate, 3)}), flush=True)
    eng.dev_free(d)
    eng.close()


if __name__ == "__main__":
    main()
