"""A circuit's key resident on the device (DESIGN.md sections 4.22 and 5.0t) on one device, one process, warmed, KZG_PERF_REPS
repetitions each (default 5) with their min-max, at n = 2^KZG_PERF_LOG (default 20), t = 3, e = 4:
  (a) wall time of kzg_circuit_quotient, gate built in: with T's coefficients and the three commitments back, without the
      coefficients, without the commitments, with neither; the same with public inputs;
  (b) the parent route on the SAME inputs: kzg_permutation_quotient with gate_coset already computed.  Producing gate_coset is NOT
      timed (the comparison favours the old route); its upload is (the old route cannot avoid it).  Both routes must return the same
      T and the same commitments, limb for limb: asserted before anything is timed;
  (c) kzg_circuit_create with and without the key's commitments.
`--kernels`: a few calls of either route and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run (k_ck_constraints
against k_pq_constraints alone).
GPU.  Writes JSON lines to profiles/r24_circuit.jsonl (or the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "5")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "20"))
SECRET = bytes(range(32))
R = K.R_MODULUS
RINV = pow(1 << 256, -1, R)
T, LOG_EXT = 3, 2


def stats(ts, scale=1e3, unit="ms"):
    return {"median_" + unit: round(scale * float(np.median(ts)), 4), "min_" + unit: round(scale * min(ts), 4),
            "max_" + unit: round(scale * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(fn):
    fn()  # warm
    return stats([timed(fn) for _ in range(REPS)])


def values(rng, rows):
    a = rng.integers(1, 1 << 64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=rows, dtype=np.uint64)
    return a


def ints(a):
    """(rows, 4) uint64 -> the integers the limbs spell (blst_fr images, not the plain values)"""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def cyclic_argument(eng, n, rng):
    """wires equal across the t columns of a row and the permutation (j, i) -> (j + 1 mod t, i): a true permutation at any size"""
    row = values(rng, n)
    shifts = [K.Scalar(pow(7, j, R)) for j in range(T)]
    sig = []
    for j in range(T):  # k_(j+1) w^i: the values of the polynomial k_(j+1) X
        c = np.zeros((n, 4), dtype=np.uint64)
        c[1] = shifts[(j + 1) % T].limbs()
        sig.append(eng.ntt_limbs(c))
    return row, np.stack([row] * T), np.stack(sig), shifts


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "r24_circuit.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    N = n * e
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    eng.set_max_batch(e - 1)  # the chunks of T go through one batched MSM on either route
    rng = np.random.default_rng(24)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    alpha, beta, gamma = (K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R) for _ in range(3))
    try:
        row, wires, sigmas, shifts = cyclic_argument(eng, n, rng)
        z, last = eng.permutation_product_limbs(wires, sigmas, shifts, beta, gamma)
        assert [int(x) for x in last] == [int(x) for x in K.Scalar(1).limbs()]
        # random selectors and public inputs; q_C closes every row.  On images: image(x y) = image(x) image(y) / 2^256
        q_lin, q_mul, pi = np.stack([values(rng, n) for _ in range(T)]), values(rng, n), values(rng, n)
        f, qs, qm, p = ints(row), [ints(c) for c in q_lin], ints(q_mul), ints(pi)
        body = [((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * RINV % R * f[i]) % R * RINV % R for i in range(n)]
        q_const = limbs([(-v) % R for v in body])             # without public inputs
        q_const_pi = limbs([(-v - p[i]) % R for i, v in enumerate(body)])
        del f, qs, qm, p, body
        circ = eng.circuit_create(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, want_key=False)
        circ_pi = eng.circuit_create(q_lin, q_mul, q_const_pi, sigmas, shifts, LOG_EXT, want_key=False)
        new = lambda **kw: circ.quotient(wires, z, alpha, beta, gamma, **kw)
        new_pi = lambda **kw: circ_pi.quotient(wires, z, alpha, beta, gamma, public_inputs=pi, **kw)
        # gate_coset for the parent route (not timed): Gate = T_gate (X^n - 1) with T_gate from the call at alpha = 0, extended
        tg, _ = circ.quotient(wires, z, K.Scalar(0), beta, gamma, want_commitments=False)
        tg = ints(tg)
        gate = limbs([((tg[k - n] if k >= n else 0) - (tg[k] if k < N - n else 0)) % R for k in range(N)])
        del tg
        gate_coset = eng.coset_extend_limbs(gate.reshape(1, N, 4), LOG_N + LOG_EXT, form=K.KZG_EXTEND_COEFFS)[0]
        old = lambda **kw: eng.permutation_quotient(wires, sigmas, z, shifts, alpha, beta, gamma, LOG_EXT, gate=gate_coset, **kw)
        if kernels_only:
            for _ in range(4):
                new(want_coeffs=False, want_commitments=False)
                old(want_coeffs=False, want_commitments=False)
            return
        c_new, p_new = new()
        c_old, p_old = old()
        c_pi, p_pi = new_pi()
        assert np.array_equal(c_new, c_old) and all(np.array_equal(a.p1, b.p1) for a, b in zip(p_new, p_old))
        assert np.array_equal(c_pi, c_old)  # the public inputs are absorbed by q_C: the same Num
        emit({"what": "routes_agree", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT,
              "T_and_commitments_equal_limb_for_limb": True})
        variants = (("call", {}), ("call_without_coefficients", {"want_coeffs": False}),
                    ("call_without_commitments", {"want_commitments": False}),
                    ("call_with_neither", {"want_coeffs": False, "want_commitments": False}))
        # interleaved, so that a drift of the machine touches both routes alike
        res = {"new": {}, "new_pi": {}, "old": {}}
        for name, kw in variants:
            for fn in (new, new_pi, old):
                fn(**kw)  # warm
            ts = {"new": [], "new_pi": [], "old": []}
            for _ in range(REPS):
                ts["new"].append(timed(lambda: new(**kw)))
                ts["old"].append(timed(lambda: old(**kw)))
                ts["new_pi"].append(timed(lambda: new_pi(**kw)))
            for k in res:
                res[k][name] = stats(ts[k])
        base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "reps": REPS}
        emit(dict(base, what="circuit_quotient", **res["new"]))
        emit(dict(base, what="circuit_quotient_with_public_inputs", **res["new_pi"]))
        emit(dict(base, what="parent_route_permutation_quotient_with_gate_coset", gate_coset_upload_MiB=N * 32 >> 20,
                  producing_gate_coset_timed=False, **res["old"]))
        circ.close()
        circ_pi.close()

        def create(want_key):
            c = eng.circuit_create(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, want_key=want_key)
            c.close()
        eng.set_max_batch(2 * T + 2)  # the key's columns in one batched MSM
        emit(dict(base, what="circuit_create", max_batch=2 * T + 2, key_MiB=((2 * T + 3) * N + 2 * (2 * T + 2) * n) * 32 >> 20,
                  without_commitments=measure(lambda: create(False)), with_commitments=measure(lambda: create(True))))
    finally:
        eng.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
