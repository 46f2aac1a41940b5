"""The product cores of csrc/field30.hip.h -- fq_mul, fq_sqr, fq_mul_sub, fq_mul_minus, fq_mul_plus, fq_sqr_minus -- return
the same digits as their definitions of before the columns became single multiply-add chains (fq_mul_sub: a b + (-c) d with c
negated once, instead of a second chain subtracted column by column).  The earlier definitions are kept verbatim in
tests/host/field30_parent_products.h; tests/host/field30_columns_host.cpp runs both on 10^5 random rows per function and on
the edges of the contracts -- every digit at +-2^29 and +-(2^29 + 4), one multiplicand a raw sum of two, values taken into
the carry pass at +-(2^31 - 1), operands at 0, +-p, +-3p -- and compares digit for digit.  The program is built and run ONCE,
under -fsanitize=undefined,address (a stand-alone g++ program: nothing is loaded into python).  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "field30_columns_host.cpp")


def test_products_match_the_earlier_definitions_digit_for_digit(tmp_path):
    exe = str(tmp_path / "field30_columns")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-DF30_COLUMNS_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all rows identical" in r.stdout
    for name in ("fq_mul", "fq_sqr", "fq_mul_sub", "fq_mul_minus", "fq_mul_plus", "fq_sqr_minus"):
        assert "%s: 100256 rows, 0 differ" % name in r.stdout
