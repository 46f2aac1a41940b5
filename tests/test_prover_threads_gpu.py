"""GPU: seven threads of prover calls on one context.

The prover calls take a feature mutex before the context's mutex -- quotient_mu (the coset extension, the quotients, the circuits),
lookup_mu (the multiplicities), fk20_mu (the Lagrange-basis openings) -- and give the context's mutex up while they copy or wait;
include/kzg_mi355x.h promises that they are as thread-safe as the other host-pointer calls.  Here they run at once: permutation
quotients of two shapes (the cached inverses of Z_H are replaced every call), quotient and opening on a resident circuit A, a
second circuit B created with its key, used and destroyed again and again, multiplicities and the lookup commitment, the
permutation commitment, an opening over the Lagrange basis and plain commitments.  Seven threads are more than a context has
slots, so reserve_slot(block=true) waits behind the feature mutexes as well.

The scenario runs in one child process under a time limit, so that a deadlock ends the child and not the suite."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 7  # ten times the child's measured wall time (the test's docstring)

CHILD = r"""
import ctypes as C, json, sys, threading, time
root = %r
sys.path[:0] = [root, root + "/oracle", root + "/tests"]
import numpy as np
import bigint_twin as BT
import circuit_oracle as CO
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import lookup_oracle as LO
import ntt_oracle as NO
import perm_quotient_oracle as PQ

R, ITERATIONS, N = PQ.R, 8, 256
ALPHA, BETA, GAMMA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 %% R, 0x1F2E3D4C5B6A79881F2E3D4C5B6A7988 %% R, 0x123456789ABCDEF0FEDCBA9876543210 %% R
ZETA, V = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE %% R, 0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A %% R
CH = [K.Scalar(x) for x in (ALPHA, BETA, GAMMA, ZETA, V)]
limbs = lambda cols: np.stack([GO.to_limbs(c) for c in cols])
raw = lambda points: b"".join(p.p1.tobytes() for p in points)

e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(1024)
e.lagrange_prepare(8)  # one basis for the three calls that commit or open over it


def argument(t, seed):
    ks = GO.shifts(t)
    wires, sigmas = GO.true_permutation(8, t, ks, seed)
    z, last = PQ.z_of(wires, sigmas, ks, BETA, GAMMA)
    assert last == 1
    return limbs(wires), limbs(sigmas), GO.to_limbs(z), [K.Scalar(k) for k in ks]


ARG = {2: argument(3, 21), 3: argument(7, 22)}  # by log_ext: e = 4 with 3 columns, e = 8 with 7


def permutation_quotient(i):
    log_ext = 2 + i %% 2
    w, s, z, ks = ARG[log_ext]
    coeffs, points = e.permutation_quotient(w, s, z, ks, *CH[:3], log_ext)
    return coeffs.tobytes() + raw(points)


def circuit(k, t, seed):
    c = CO.satisfied(k, t, seed, True)
    z, last = CO.z_of(c, BETA, GAMMA)
    assert last == 1
    return c, limbs(c.wires), GO.to_limbs(z), GO.to_limbs(c.pi)


def create(c, log_ext, want_key):
    return e.circuit_create(limbs(c.q_lin), GO.to_limbs(c.q_mul), GO.to_limbs(c.q_const), limbs(c.sigmas), [K.Scalar(k) for k in c.ks],
                            log_ext, want_key=want_key)


CA, WA, ZA, PA = circuit(8, 3, 31)
CB, WB, ZB, PB = circuit(6, 7, 32)
A = create(CA, 2, False)


def circuit_a(i):
    t_coeffs, points = A.quotient(WA, ZA, *CH[:3], public_inputs=PA)
    (abar, sbar, zw), proof = A.open(WA, ZA, t_coeffs, *CH, public_inputs=PA)
    return t_coeffs.tobytes() + raw(points + [proof]) + b"".join(x.limbs().tobytes() for x in abar + sbar + [zw])


def circuit_b(i):
    B = create(CB, 3, True)
    try:
        t_coeffs, points = B.quotient(WB, ZB, *CH[:3], public_inputs=PB)
    finally:
        B.close()
    return raw(B.key + points) + t_coeffs.tobytes()


LOOKUPS, TABLE, MULT = LO.valid_lookup(N, 2, 41)
LF, LT = limbs(LOOKUPS), GO.to_limbs(TABLE)


def lookup(i):
    mult, rows = e.lookup_multiplicities(LT, LF)
    point, phi, last = e.lookup_commit(LF, LT, mult, CH[1])
    return mult.tobytes() + rows.tobytes() + raw([point]) + phi.tobytes() + last.tobytes()


def permutation_commit(i):
    w, s, z, ks = ARG[2]
    point, z, last = e.permutation_commit(w, s, ks, CH[1], CH[2])
    return raw([point]) + z.tobytes() + last.tobytes()


rnd = __import__("random").Random(51)
EVALS = [rnd.randrange(R) for _ in range(N)]
OPEN = GO.to_limbs(EVALS), K.Scalar(ZETA), K.Scalar(NO.barycentric_eval(EVALS, ZETA))
POLY = GO.to_limbs([rnd.randrange(R) for _ in range(1024)])


def open_lagrange(i):
    return raw([e.open_lagrange_limbs(*OPEN)])


def commit(i):
    return raw([e.commit_limbs(POLY)])


CALLS = [permutation_quotient, circuit_a, circuit_b, lookup, permutation_commit, open_lagrange, commit]
want = {f.__name__: [f(0), f(1)] for f in CALLS}  # single-threaded
assert MULT == GO.from_limbs(np.frombuffer(want["lookup"][0][:N * 32], dtype=np.uint64))
problems = []


def worker(f):
    for i in range(ITERATIONS):
        try:
            if f(i) != want[f.__name__][i %% 2]:
                problems.append({"thread": f.__name__, "iteration": i, "what": "differs from the single-threaded bytes"})
        except Exception as ex:  # noqa: BLE001
            problems.append({"thread": f.__name__, "iteration": i, "what": repr(ex)})
            return


threads = [threading.Thread(target=worker, args=(f,)) for f in CALLS]
t0 = time.time()
for th in threads:
    th.start()
for th in threads:
    th.join()
wall = time.time() - t0
for f in CALLS:  # the context still serves one call of each kind
    if f(0) != want[f.__name__][0]:
        problems.append({"thread": f.__name__, "iteration": "after the join", "what": "differs from the single-threaded bytes"})
gone = C.c_void_p(A._c.value)
A.close()
rc = K.load_library().kzg_circuit_destroy(e._h, gone)
if rc != K.KZG_ERR_INVALID_ARG:
    problems.append({"thread": "main", "iteration": "after the join", "what": "kzg_circuit_destroy of a destroyed handle returned %%d" %% rc})
e.close()
print("threads ran for %%.2f s" %% wall, file=sys.stderr)
print(json.dumps(problems))
"""


def test_seven_threads_of_prover_calls_on_one_context():
    """Every iteration of every thread returns the bytes the same call returned single-threaded; afterwards the context serves one
    call of each kind and a destroyed circuit's handle is refused.

    The child -- interpreter start, imports, the SRS, the inputs from the big-integer oracles, the single-threaded pass, 7 x 8
    threaded iterations, the calls after the join -- took 0.66 s of wall time on an MI355X.  Its limit is ten times that, 7 s: the
    threads contend for the machine's CPUs and for the context's slots."""
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert p.returncode == 0, p.stderr[-3000:]
    print(p.stderr.strip().splitlines()[-1])  # "threads ran for .. s"
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [], p.stderr[-1000:]
