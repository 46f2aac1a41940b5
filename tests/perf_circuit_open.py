"""The last round of a circuit's proof (DESIGN.md sections 4.23 and 5.0u) on one device, one process, warmed, KZG_PERF_REPS
alternated repetitions (default 9) with their min-max, at n = 2^KZG_PERF_LOG (default 20), t = 3, e = 4, on resident inputs:
  (a) kzg_circuit_open_device: wires, z, PI and T (from kzg_circuit_quotient_device) never leave the device;
  (b) the floor the call cannot beat: kzg_open_sets_submit + kzg_wait_sets alone on a precomputed resident stack of the same 2 t + 1
      polynomials (r included).  The two proofs must be equal bit for bit: asserted before anything is timed.  (a) - (b) is the cost
      of linearising: t + 2 inverse transforms, the evaluations, two waits;
  (c) the piece-wise route available without the call: download the key's 2 t + 2 coefficient columns, the evaluations and r on the
      host (tests/host/lin_cpu_port.cpp, 16 threads, run apart and added), kzg_open_sets on host pointers (which uploads the stack).
      The wires' and z's coefficients, which that route also needs on the host, are NOT timed (the comparison favours it);
  (d) with kzg_set_timing: the events around the two launches of k_lin_combine + k_lin_finish (zeta: 3 t + e + 2 columns, zeta w:
      one) and their algorithmic bytes per second (every column read once, both sums written once).
GPU.  Writes JSON lines to profiles/r25_circuit_open.jsonl (or the path given) and prints them."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

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
THREADS = 16


def cpu_port(log_n):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "lin_cpu_port")
        subprocess.run(["g++", "-O2", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "lin_cpu_port.cpp")], check=True)
        out = subprocess.run([exe, str(log_n), str(LOG_EXT), str(T), str(THREADS), str(REPS)], capture_output=True, text=True,
                             check=True).stdout.split("\n")
    rows = [[float(x) for x in line.split()] for line in out[:REPS]]
    return [r[0] for r in rows], [r[1] for r in rows]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r25_circuit_open.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    N = n * e
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n)
    lib = K.load_library()
    rng = np.random.default_rng(25)
    lines, bufs = [], []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def up(a):
        a = np.ascontiguousarray(a)
        bufs.append(eng.dev_alloc(a.nbytes))
        eng.dev_upload(bufs[-1], a)
        return bufs[-1]

    def down(dptr, rows, into=None):
        got = np.zeros((rows, 4), dtype=np.uint64) if into is None else into
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
        circ.quotient_device(d_w, d_z, alpha, beta, gamma, d_t, d_public_inputs=d_pi)
        new = lambda: circ.open_device(d_w, d_z, d_t, alpha, beta, gamma, zeta, v, d_public_inputs=d_pi)
        evals, proof = new()
        # the stack of the same opening, resident: r from the test hook, the coefficients by the library's transforms
        _, r = circ.linearise(wires, z, down(d_t, N - n), alpha, beta, gamma, zeta, public_inputs=pi)
        sig = [down(circ.column_device(K.KZG_CIRCUIT_COL_SIGMA + j, K.KZG_CIRCUIT_COEFFS)[0], n) for j in range(T - 1)]
        stack = [r] + [eng.intt_limbs(wires[j]) for j in range(T)] + sig + [eng.intt_limbs(z)]
        stack = np.ascontiguousarray(np.stack(stack))  # (2 t + 1, n, 4)
        d_stack = up(stack)
        set_of = [0] * (2 * T) + [1]
        sets = [[zeta], [K.Scalar(zeta.v * K.domain_root(LOG_N).v % R)]]

        def floor():
            eng.open_sets_submit(0, d_stack, n, 2 * T + 1, set_of, sets, v)
            return eng.wait_sets(0, set_of, sets)
        ys, want = floor()
        assert np.array_equal(proof.p1, want.p1)
        assert [a.v for a in evals[0]] + [s.v for s in evals[1]] + [evals[2].v] == [row_[0].v for row_ in ys[1:]] and ys[0][0].v == 0
        emit({"what": "routes_agree", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "proof_equal_bit_for_bit": True})
        key_host = np.zeros(((2 * T + 2) * n, 4), dtype=np.uint64)
        key_ptr = circ.column_device(K.KZG_CIRCUIT_COL_QLIN, K.KZG_CIRCUIT_COEFFS)[0]

        def piece():  # without the host arithmetic, which lin_cpu_port times apart
            down(key_ptr, (2 * T + 2) * n, key_host)
            return eng.open_sets_limbs(stack, set_of, sets, v)
        assert np.array_equal(piece()[1].p1, want.p1)
        ts = {"new": [], "floor": [], "piece": []}
        for _ in range(REPS):  # alternated, so that a drift of the machine touches the routes alike
            ts["new"].append(PC.timed(new))
            ts["floor"].append(PC.timed(floor))
            ts["piece"].append(PC.timed(piece))
        cpu_ev, cpu_r = cpu_port(LOG_N)
        base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "reps": REPS}
        emit(dict(base, what="circuit_open_device", **PC.stats(ts["new"])))
        emit(dict(base, what="open_sets_submit_on_a_precomputed_stack", polynomials=2 * T + 1, **PC.stats(ts["floor"])))
        emit(dict(base, what="cost_of_linearising_ms", median=round(1e3 * float(np.median(ts["new"]) - np.median(ts["floor"])), 4)))
        emit(dict(base, what="piecewise_route", download_and_open_sets=PC.stats(ts["piece"]), cpu_threads=THREADS,
                  cpu_evaluations=PC.stats(cpu_ev), cpu_r=PC.stats(cpu_r), wire_and_z_coefficients_on_the_host_timed=False,
                  total_median_ms=round(1e3 * float(np.median(ts["piece"]) + np.median(cpu_ev) + np.median(cpu_r)), 4)))
        eng.set_timing(True)
        ms = []
        for _ in range(REPS):
            new()
            ms.append(eng.combine_ms(0) * 1e-3)
        eng.set_timing(False)
        cols = 3 * T + e + 2 + 1
        nbytes = (cols + 2) * n * 32
        emit(dict(base, what="k_lin_combine_and_finish_both_points", columns_read=cols, sums_written=2, algorithmic_MiB=nbytes >> 20,
                  algorithmic_GB_per_s=round(nbytes / float(np.median(ms)) / 1e9, 1), **PC.stats(ms)))
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
