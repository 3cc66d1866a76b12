"""The twist table of the N = 2048 Solinas plan restated in Python (rows and lane-pair twiddles of the forward and
the inverse body), shared by tests/test_tw_codegen.py (the emulated asm bodies read it) and
tests/test_plan_tables_host.py (csrc/ntt64_plan_tables.hpp must produce the same words)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001


def tables(oracle):
    plan = oracle.Plan.try_new(2048, P)
    tw = [int(v) for v in plan.twid]
    br = lambda x, b: int(format(x, f"0{b}b")[::-1], 2)
    psi = tw[br(1, 11)]
    omega = pow(psi, 64, P)
    f, i = [], []
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_tw_kernel as G
    # the forward bodies' scale plan, folded into the twist table as ntt64_plan_tables.hpp twist_table does
    tabs = G.load_tables()
    g1_out, cyc_in = tabs["TW_G1_OUT_SCALE"][0], tabs["TW_CYC_IN_SCALE"][0]
    for blk in range(32):
        rho = pow(psi, 2 * br(blk, 5) + 1, P)
        rinv = pow(rho, P - 2, P)
        f += [pow(rho, j, P) * pow(2, (cyc_in[j >> 1] - g1_out[blk]) % 192, P) % P for j in range(64)]
        i += [pow(rinv, j, P) for j in range(64)]
    f += [pow(omega, br(g, 5), P) for g in range(32)]
    i += [pow(pow(omega, br(g, 5), P), P - 2, P) for g in range(32)]
    return plan, f, i
