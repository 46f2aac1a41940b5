"""Every kernel of circuit_verify_kernels.hip is listed here with what the compiler gives it for gfx950:
no scratch memory, no spilled vector register (a scalar register spilled goes to a lane of a vector register, not to memory;
the count is printed), and a VGPR count within the project's goal of 160 for light kernels -- or an entry in
EXCEPTIONS with the reason.  The counts are read from the compiler's resource metadata, compiled with the Makefile's flags
through tests/isa_cache.py, and printed; none is fixed here.  CPU only (hipcc cross-compiles)."""
from isa_cache import kernel_meta, requires_hipcc

UNIT = "circuit_verify_kernels.hip"
KERNELS = ("k_cvb_publicE", "k_cvb_linE", "k_cvb_scalarsE", "k_cvb_key_splitE", "k_cvb_stage2E")  # ("E": the end of the mangled name)
GOAL = 160
# above the goal on purpose
EXCEPTIONS = {
    "k_cvb_stage2E": "a 128-step GLV ladder on an XYZZ point, the loop of k_vc_cell_scale and k_vc_ladder (verify_kernels.hip): "
                     "latency-bound, one dependent chain per lane, with the point, phi(point), their sum and the accumulator live "
                     "(16 field elements of 13 digits); it takes the registers it needs, as those kernels do",
    "k_cvb_linE": "one lane per proof with beta, gamma, alpha, zeta, zeta^n, A, B and L_0(zeta) live across the loop over the wires "
                  "(eight Fr values of nine digits beside a product's forty registers); it runs M / 64 workgroups once a call, "
                  "before any ladder, and shares the chip with nothing of this call",
}


@requires_hipcc
def test_every_kernel_of_the_unit_is_listed_without_scratch_and_within_the_goal_or_excepted():
    meta = kernel_meta(UNIT)
    assert len(meta) == len(KERNELS), sorted(meta)  # a kernel added to the unit is added here
    for kernel in KERNELS:
        found = [k for k in meta if kernel in k]
        assert len(found) == 1, (kernel, sorted(meta))
        m = meta[found[0]]
        print(found[0], "vgpr", m["vgpr_count"], "agpr", m.get("agpr_count"), "sgpr", m.get("sgpr_count"), "sgpr spilled", m["sgpr_spill_count"])
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (kernel, m)
        if kernel in EXCEPTIONS:
            assert GOAL < m["vgpr_count"] <= 512, (kernel, m)  # an exception that is no longer one leaves the list
        else:
            assert m["vgpr_count"] <= GOAL, (kernel, m)
    assert set(EXCEPTIONS) <= set(KERNELS)
