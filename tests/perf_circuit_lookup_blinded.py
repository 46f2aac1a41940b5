"""kzg_circuit_lookup_prove_blinded_device (DESIGN.md sections 4.30 and 5.0ac) against kzg_circuit_lookup_prove_device on the SAME
circuit handle: one device, one process, warmed, five alternated repetitions (KZG_PERF_REPS) with their min-max, at
n = 2^KZG_PERF_LOG (default 20), t = 3, c = 3, e = 4 (D = 3 n + 6 < 4 n), resident wires, 16 public inputs, a host clock around
synchronous calls.  The witness and the table are tests/perf_circuit_lookup.py's; the SRS has n + t + 3 points.  Before anything is
timed both proofs are checked with the one verifier, kzg_circuit_lookup_verify_proof.
`--kernels` (`--kernels-plain`): four blinded (plain) lookup proofs and nothing else, for separate `rocprofv3 --kernel-trace --stats`
runs whose kernel_stats.csv are compared kernel by kernel.
GPU.  Writes JSON lines to profiles/r35_circuit_lookup_blinded.jsonl (or the path given) and prints them."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import perf_circuit as PC  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "5")), 5)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "20"))
R = K.R_MODULUS
T, LOG_EXT, C_TAB, N_PUBLIC = PC.T, PC.LOG_EXT, 3, 16


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "blinded" if "--kernels" in sys.argv else ("plain" if "--kernels-plain" in sys.argv else None)
    out = args[0] if args else os.path.join(ROOT, "profiles", "r35_circuit_lookup_blinded.jsonl")
    n = 1 << LOG_N
    num_blinders, quotient_len = K.circuit_lookup_blinded_sizes(n, T, LOG_EXT, C_TAB)
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n + T + 3)
    rng = np.random.default_rng(31)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    d_w = None
    try:
        row, wires, sigmas, shifts = PC.cyclic_argument(eng, n, rng)
        q_lin, q_mul, pi = np.stack([PC.values(rng, n) for _ in range(T)]), PC.values(rng, n), PC.values(rng, n)
        pi[N_PUBLIC:] = 0
        f, qs, qm, p = PC.ints(row), [PC.ints(c) for c in q_lin], PC.ints(q_mul), PC.ints(pi)
        q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                            for i in range(n)])
        del f, qs, qm, p
        q_k = np.zeros((n, 4), dtype=np.uint64)
        q_k[:n // 2] = K.Scalar(1).limbs()
        col = row.copy()
        col[n // 2:] = 0  # the zero tuple
        table = np.stack([col] * C_TAB)
        circ = eng.circuit_create_lookup(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, table, q_k, want_key=True)
        d_w = eng.dev_alloc(wires.nbytes)
        eng.dev_upload(d_w, np.ascontiguousarray(wires))
        pub_rows = np.ascontiguousarray(pi[:N_PUBLIC])
        blinders = K.circuit_lookup_blinders(T, LOG_EXT)
        assert blinders.shape[0] == num_blinders

        def prove_blinded():
            return circ.lookup_prove_blinded_device(d_w, blinders, pub_rows)

        def prove_plain():
            return circ.lookup_prove_device(d_w, pub_rows)

        if kernels_only:
            for _ in range(4):
                prove_plain() if kernels_only == "plain" else prove_blinded()
            return
        g1, g2 = eng.srs_read(0, 1), np.stack([K.srs_g2_at(PC.SECRET, j) for j in range(3)])
        public = [K.Scalar.from_limbs(x) for x in pub_rows]
        blinded, plain = prove_blinded(), prove_plain()
        assert blinded != plain and len(blinded) == len(plain)
        assert K.circuit_lookup_verify_proof(circ.key, n, LOG_EXT, C_TAB, shifts, public, blinded, g1, g2)
        assert K.circuit_lookup_verify_proof(circ.key, n, LOG_EXT, C_TAB, shifts, public, plain, g1, g2)
        emit({"what": "proofs_verify", "measured": True, "log_n": LOG_N, "t": T, "c": C_TAB, "log_ext": LOG_EXT, "n_public": N_PUBLIC,
              "blinders": num_blinders, "quotient_len": quotient_len})
        prove_blinded(), prove_plain()  # warm
        ts = {"blinded": [], "plain": []}
        for _ in range(REPS):  # alternated
            ts["blinded"].append(PC.timed(prove_blinded))
            ts["plain"].append(PC.timed(prove_plain))
        base = {"measured": True, "log_n": LOG_N, "t": T, "c": C_TAB, "log_ext": LOG_EXT, "reps": REPS, "n_public": N_PUBLIC,
                "proof_bytes": K.circuit_lookup_proof_size(T, LOG_EXT, C_TAB)}
        emit(dict(base, what="circuit_lookup_prove_blinded_device", **PC.stats(ts["blinded"])))
        emit(dict(base, what="circuit_lookup_prove_device_same_handle", **PC.stats(ts["plain"])))
        circ.close()
    finally:
        if d_w is not None:
            eng.dev_free(d_w)
        eng.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
