"""Batched NTT against the loop over columns: kzg_ntt_batch_device (one launch per pass for the whole batch, k_nttb_pass) and
`batch` calls of kzg_ntt_device (one launch per column and pass, k_ntt_pass), for batch in {1, 4, 8} at 2^12, 2^16 and 2^20 values,
both directions, device buffers.  Both are synchronous calls, so a figure holds the host round trip of each call: one for the
batch, `batch` for the loop.  Three repetitions of the whole table in one process, each the median of KZG_PERF_REPS (40) timed
calls after three warm-up calls; min - max over the repetitions.  GPU; prints JSON lines."""
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


def median_us(call, reps):
    for _ in range(3):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def main():
    reps = int(os.environ.get("KZG_PERF_REPS", "40"))
    eng = K.Engine(0)
    rows = {}
    for rep in range(3):
        for k in (12, 16, 20):
            n = 1 << k
            for batch in (1, 4, 8):
                d_in, d_out = eng.dev_alloc(batch * n * 32), eng.dev_alloc(batch * n * 32)
                eng.dev_upload(d_in, random_images(batch * n, k + batch))
                for inverse in (False, True):
                    def loop():
                        for b in range(batch):
                            eng.ntt_device(d_in + 32 * b * n, d_out + 32 * b * n, n, inverse)

                    batched = median_us(lambda: eng.ntt_batch_device(d_in, n, batch, n, d_out, n, inverse), reps)
                    looped = median_us(loop, reps)
                    rows.setdefault((k, batch, inverse), []).append((batched, looped))
                eng.dev_free(d_in)
                eng.dev_free(d_out)
    for (k, batch, inverse), v in sorted(rows.items()):
        b, l = [x[0] for x in v], [x[1] for x in v]
        print(json.dumps({"log_n": k, "batch": batch, "direction": "inverse" if inverse else "forward", "per": "synchronous call", "reps": reps, "repetitions": len(v),
                          "batched_us_min": round(min(b), 1), "batched_us_max": round(max(b), 1),
                          "loop_us_min": round(min(l), 1), "loop_us_max": round(max(l), 1),
                          "loop_over_batched_min": round(min(x[1] / x[0] for x in v), 3),
                          "loop_over_batched_max": round(max(x[1] / x[0] for x in v), 3)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
