"""The blinded rounds of a circuit's proof (DESIGN.md sections 4.24 and 5.0w) on one device, one process, warmed, KZG_PERF_REPS
alternated repetitions (default 9) with their min-max, at n = 2^KZG_PERF_LOG (default 20), t = 3, e = 4, on resident inputs and the
same witness:
  (a) kzg_circuit_quotient_blinded_device (without commitments) against kzg_circuit_quotient_device;
  (b) kzg_circuit_open_blinded_device against kzg_circuit_open_device;
  (c) with kzg_set_timing: the events around the last round's sums (k_lin_combine + k_lin_finish per point, with blinders also
      k_blind_tail per point), blinded against plain.
Before anything is timed: with all blinders zero the blinded calls return the plain calls' coefficients and proof bit for bit.
The patch and tail kernels' own times come from a run of this script under a kernel trace (KZG_PERF_REPS=3 is enough): they are
too short for host clocks.
GPU.  Writes JSON lines to profiles/r28_circuit_blinded.jsonl (or the path given) and prints them."""
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

REPS = max(int(os.environ.get("KZG_PERF_REPS", "9")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "20"))
R = K.R_MODULUS
T, LOG_EXT = PC.T, PC.LOG_EXT


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r28_circuit_blinded.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    N = n * e
    LT = (e - 1) * n + T + 3
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n + T + 3)
    lib = K.load_library()
    rng = np.random.default_rng(28)
    lines, bufs = [], []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def up(a):
        a = np.ascontiguousarray(a)
        bufs.append(eng.dev_alloc(a.nbytes))
        eng.dev_upload(bufs[-1], a)
        return bufs[-1]

    def down(dptr, rows):
        got = np.zeros((rows, 4), dtype=np.uint64)
        assert lib.kzg_dev_download(eng._h, got.ctypes.data, C.c_void_p(dptr), rows * 32) == 0
        return got

    alpha, beta, gamma, zeta, v = (K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R) for _ in range(5))
    try:
        row, wires, sigmas, shifts = PC.cyclic_argument(eng, n, rng)
        z, last = eng.permutation_product_limbs(wires, sigmas, shifts, beta, gamma)
        q_lin, q_mul, pi = np.stack([PC.values(rng, n) for _ in range(T)]), PC.values(rng, n), PC.values(rng, n)
        f, qs, qm, p = PC.ints(row), [PC.ints(c) for c in q_lin], PC.ints(q_mul), PC.ints(pi)
        q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                            for i in range(n)])
        del f, qs, qm, p
        circ = eng.circuit_create(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, want_key=False)
        d_w, d_z, d_pi = up(wires), up(z), up(pi)
        bufs.append(eng.dev_alloc((N - n) * 32))
        d_t = bufs[-1]
        bufs.append(eng.dev_alloc(LT * 32))
        d_tb = bufs[-1]
        blinders, zero = circ.blinders(), np.zeros((2 * T + 3 + e - 2, 4), dtype=np.uint64)

        def quot_plain():
            circ.quotient_device(d_w, d_z, alpha, beta, gamma, d_t, d_public_inputs=d_pi)

        def quot_blind(b=blinders):
            circ.quotient_blinded_device(d_w, d_z, alpha, beta, gamma, b, d_tb, d_public_inputs=d_pi, want_commitments=False)

        def open_plain():
            return circ.open_device(d_w, d_z, d_t, alpha, beta, gamma, zeta, v, d_public_inputs=d_pi)

        def open_blind(b=blinders):
            return circ.open_blinded_device(d_w, d_z, d_tb, alpha, beta, gamma, zeta, v, b, d_public_inputs=d_pi)

        # all blinders zero: the plain calls' outputs bit for bit
        quot_plain()
        quot_blind(zero)
        plain_t, blind_t = down(d_t, N - n), down(d_tb, LT)
        assert np.array_equal(blind_t[:N - n], plain_t) and not blind_t[N - n:].any()
        (ev0, pr0), (ev1, pr1) = open_plain(), open_blind(zero)
        assert np.array_equal(pr0.p1, pr1.p1) and [x.v for x in ev0[0]] == [x.v for x in ev1[0]] and ev0[2].v == ev1[2].v
        emit({"what": "zero_blinders_give_the_plain_outputs", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT,
              "coefficients_and_proof_equal_bit_for_bit": True})
        quot_blind()
        open_blind()  # warm, and d_tb holds the blinded quotient of `blinders`
        ts = {"quot_plain": [], "quot_blind": [], "open_plain": [], "open_blind": []}
        for _ in range(REPS):  # alternated, so that a drift of the machine touches the routes alike
            ts["quot_plain"].append(PC.timed(quot_plain))
            ts["quot_blind"].append(PC.timed(quot_blind))
            ts["open_plain"].append(PC.timed(open_plain))
            ts["open_blind"].append(PC.timed(open_blind))
        base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "reps": REPS}
        emit(dict(base, what="circuit_quotient_device", **PC.stats(ts["quot_plain"])))
        emit(dict(base, what="circuit_quotient_blinded_device", commitments=False, **PC.stats(ts["quot_blind"])))
        emit(dict(base, what="circuit_open_device", **PC.stats(ts["open_plain"])))
        emit(dict(base, what="circuit_open_blinded_device", **PC.stats(ts["open_blind"])))
        emit(dict(base, what="blinded_minus_plain_median_ms",
                  quotient=round(1e3 * float(np.median(ts["quot_blind"]) - np.median(ts["quot_plain"])), 4),
                  open=round(1e3 * float(np.median(ts["open_blind"]) - np.median(ts["open_plain"])), 4)))
        eng.set_timing(True)
        ms = {"plain": [], "blind": []}
        for _ in range(REPS):
            open_plain()
            ms["plain"].append(eng.combine_ms(0) * 1e-3)
            open_blind()
            ms["blind"].append(eng.combine_ms(0) * 1e-3)
        eng.set_timing(False)
        emit(dict(base, what="last_round_sums_both_points", plain=PC.stats(ms["plain"]), blinded_with_k_blind_tail=PC.stats(ms["blind"])))
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
