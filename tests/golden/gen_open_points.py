#!/usr/bin/env python3
"""Generates tests/golden/open_points.json: multiproofs (one proof for P at k points) from oracle/bigint_twin.py
(Python big ints only), by the known-secret shortcut

    proof = [(P(s) - I(s)) / Z(s)]G1,   Z = prod (X - z_i),   I = the interpolant of (z_i, P(z_i)),

with I(s) in Lagrange form.  Inputs: the reference's bench polynomial of each degree (c_i = 5^i + 10), the bench secret,
and the points z_i = (bench input point of the degree) + i.
Run:  python tests/golden/gen_open_points.py   (about a minute; rewrites open_points.json)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bigint_twin as T  # noqa: E402

R = T.R
S = T.fr_from_be_bytes(T.BENCH_SECRET_BE)


def case(degree, k):
    c = T.bench_coefficients(degree)
    zs = [(T.bench_input_point(degree) + i) % R for i in range(k)]
    ys = [T.poly_evaluate(c, z) for z in zs]
    zv, iv = 1, 0
    for z in zs:
        zv = zv * (S - z) % R
    for i, zi in enumerate(zs):
        num, den = 1, 1
        for j, zj in enumerate(zs):
            if j != i:
                num, den = num * (S - zj) % R, den * (zi - zj) % R
        iv = (iv + ys[i] * num * pow(den, R - 2, R)) % R
    ps = T.poly_evaluate(c, S)
    proof = T.g1_mul(T.G1, (ps - iv) * pow(zv, R - 2, R) % R)
    return {"degree": degree, "k": k, "zs": [hex(z) for z in zs], "ys": [hex(y) for y in ys],
            "commitment": T.g1_compress(T.g1_mul(T.G1, ps)).hex(), "proof": T.g1_compress(proof).hex()}


def main():
    cases = [case(d, k) for d in (1 << 10, 1 << 16, 1 << 20) for k in (2, 16, 64)]
    with open(os.path.join(HERE, "open_points.json"), "w") as f:
        json.dump({"secret_be": T.BENCH_SECRET_BE.hex(), "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
