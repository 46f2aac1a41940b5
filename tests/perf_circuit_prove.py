"""kzg_circuit_prove_device (DESIGN.md sections 4.25 and 5.0x) against the existing device-pointer calls chained by hand, one
device, one process, warmed, three alternated repetitions (KZG_PERF_REPS) with their min-max, at n = 2^KZG_PERF_LOG (default 20),
t = 3, e = 4, resident wires, public inputs, a host clock around synchronous calls:
  (a) the plain proof in one call;
  (b) the plain chain: t + 1 kzg_commit_evaluations_submit / kzg_wait, kzg_permutation_product_device, kzg_circuit_quotient_device,
      e - 1 kzg_commit_submit / kzg_wait on T's chunks, kzg_circuit_open_device -- with fixed challenges, so without any hashing;
  (c) the same chain with the evaluation pass a hashing caller needs before it knows v: on resident inputs that is a second
      kzg_circuit_open_device under a placeholder v (kzg_circuit_linearise takes host pointers);
  (d) the blinded proof in one call (its chain has no device-pointer form for the blinded commitments and is not timed);
  (e) kzg_circuit_proof_challenges alone on the same statement: the host's share for the transcript (the public inputs are hashed).
Everything is taken twice: with n public inputs (the witness of tests/perf_circuit.py has a full column of them; the transcript then
hashes 32 n bytes and the call uploads them) and with 16, the rest of the column zero.
The chain's entry points are this tree's: the parent commit's code for them is unchanged.  Before anything is timed the proofs are
checked with kzg_circuit_verify_proof.  GPU.  Writes JSON lines to profiles/r29_circuit_prove.jsonl (or the path given)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import perf_circuit as PC  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "3")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "20"))
R = K.R_MODULUS
T, LOG_EXT = PC.T, PC.LOG_EXT


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r29_circuit_prove.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    N = n * e
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n + T + 3)
    rng = np.random.default_rng(29)
    lines, bufs = [], []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def up(a):
        a = np.ascontiguousarray(a)
        bufs.append(eng.dev_alloc(a.nbytes))
        eng.dev_upload(bufs[-1], a)
        return bufs[-1]

    alpha, beta, gamma, zeta, v = (K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R) for _ in range(5))
    try:
        row, wires, sigmas, shifts = PC.cyclic_argument(eng, n, rng)
        q_lin, q_mul, pi_full = np.stack([PC.values(rng, n) for _ in range(T)]), PC.values(rng, n), PC.values(rng, n)
        d_w, d_s = up(wires), up(sigmas)
        bufs.append(eng.dev_alloc(n * 32))
        d_z = bufs[-1]
        bufs.append(eng.dev_alloc((N - n) * 32))
        d_t = bufs[-1]
        bufs.append(eng.dev_alloc(n * 32))
        d_pi = bufs[-1]
        for n_public in (n, 16):
            pi = pi_full.copy()
            pi[n_public:] = 0
            eng.dev_upload(d_pi, pi)
            f, qs, qm, p = PC.ints(row), [PC.ints(c) for c in q_lin], PC.ints(q_mul), PC.ints(pi)
            q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                                for i in range(n)])
            del f, qs, qm, p
            circ = eng.circuit_create(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, want_key=True)
            blinders = circ.blinders()
            pub_rows = np.ascontiguousarray(pi[:n_public])

            def prove_plain():
                return circ.prove_device(d_w, pub_rows, None)

            def prove_blind():
                return circ.prove_device(d_w, pub_rows, blinders)

            def chain(extra_pass):
                for j in range(T):
                    eng.commit_evaluations_submit(0, d_w + 32 * j * n, n)
                    eng.wait(0)
                eng.permutation_product_device(d_w, d_s, n, T, shifts, beta, gamma, d_z)
                eng.commit_evaluations_submit(0, d_z, n)
                eng.wait(0)
                circ.quotient_device(d_w, d_z, alpha, beta, gamma, d_t, d_public_inputs=d_pi)
                for k in range(e - 1):
                    eng.commit_submit(0, d_t + 32 * k * n, n)
                    eng.wait(0)
                if extra_pass:
                    circ.open_device(d_w, d_z, d_t, alpha, beta, gamma, zeta, K.Scalar(1), d_public_inputs=d_pi)
                return circ.open_device(d_w, d_z, d_t, alpha, beta, gamma, zeta, v, d_public_inputs=d_pi)

            # the verifier takes [s^0]G1 and three G2 points
            g1, g2 = eng.srs_read(0, 1), np.stack([K.srs_g2_at(PC.SECRET, j) for j in range(3)])
            key_rows = np.ascontiguousarray(np.stack([c.p1 for c in circ.key]), dtype=np.uint64)
            shift_rows = np.ascontiguousarray(np.stack([k.limbs() for k in shifts]))
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            lib = K.load_library()
            for proof in (prove_plain(), prove_blind()):
                buf, ok = np.frombuffer(proof, dtype=np.uint8), C.c_int(0)
                assert lib.kzg_circuit_verify_proof(ptr(key_rows), n, T, LOG_EXT, ptr(shift_rows), ptr(pub_rows), n_public, ptr(buf), len(proof),
                                                    ptr(g1), 144, ptr(g2), 288, C.byref(ok)) == 0 and ok.value == 1
            emit({"what": "proofs_verify", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "n_public": n_public})
            last = np.frombuffer(prove_plain(), dtype=np.uint8)
            five = np.zeros((5, 4), dtype=np.uint64)

            def transcript():
                assert lib.kzg_circuit_proof_challenges(ptr(key_rows), n, T, LOG_EXT, ptr(shift_rows), ptr(pub_rows), n_public, ptr(last), len(last),
                                                        ptr(five)) == 0
            prove_plain(), prove_blind(), chain(True)  # warm
            ts = {"prove_plain": [], "chain": [], "chain_extra_pass": [], "prove_blind": [], "transcript": []}
            for _ in range(REPS):  # alternated
                ts["prove_plain"].append(PC.timed(prove_plain))
                ts["chain"].append(PC.timed(lambda: chain(False)))
                ts["chain_extra_pass"].append(PC.timed(lambda: chain(True)))
                ts["prove_blind"].append(PC.timed(prove_blind))
                ts["transcript"].append(PC.timed(transcript))
            base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "reps": REPS, "n_public": n_public}
            emit(dict(base, what="circuit_prove_device_plain", **PC.stats(ts["prove_plain"])))
            emit(dict(base, what="plain_chain_of_device_calls_fixed_challenges", **PC.stats(ts["chain"])))
            emit(dict(base, what="plain_chain_with_the_extra_evaluation_pass", **PC.stats(ts["chain_extra_pass"])))
            emit(dict(base, what="circuit_prove_device_blinded", **PC.stats(ts["prove_blind"])))
            emit(dict(base, what="circuit_proof_challenges_host_only", **PC.stats(ts["transcript"])))
            circ.close()
    finally:
        for b in bufs:
            eng.dev_free(b)
        eng.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
