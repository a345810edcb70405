"""Generates scripts/valu_probe11.hip: under the priority windows, is rotr16 better written as
v_xor_b32 + v_alignbit_b32 than as the two SDWA xors?

probe10 found that with the half-rate runs (H: v_add3, SDWA xor, v_alignbit) at s_setprio 1 and
the full-rate runs (F: v_add_u32, v_xor_b32) at 0, a wave inside an F run only fills what the
other waves' H ops leave free.  A half-round (4 G) then costs about max(4 H, 2 (H + F)) cycles
per wave instead of a weighted sum: the H ops alone, until the issue port binds.  The kernels'
G has H = 28, F = 20 per half-round (bound 112 cycles); the SDWA pair was chosen when all 48
slots counted.  xor + alignbit is 1 F + 1 H, which makes H = 24, F = 24 with the same 48 ops
(bound 96 cycles).  The blocks are gen_valu_probe9's round robin of 4 columns from registers
v8..v35, the harness is gen_valu_probe10's.  Arms:
  0  the kernels' windowed block (probe10's arm 3), the control
  1  rotr16 as v_xor_b32 + v_alignbit_b32 x, x, 16; the new xor run at priority 0 in a window of
     its own: H8 F4 H4 F8 H8 F4 H4 F8 around the loop, 8 s_setprio per block
  2  the same ops, the new xor run left inside the priority-1 window around it (6 s_setprio)
  3  arm PERM_OF with v_perm_b32 (selector in an SGPR) for the half swap
  4  arm 1's ops with no s_setprio: is a gain from the windows or from the ops?
Every arm has 48 VALU ops per block, so T lane-ops/s and blocks/s compare directly.  Readings
at 5 (k_cas_sampled_lanes today), 6 (at 80 VGPRs) and 8 waves/SIMD, as probe10 takes them, with
the board power beside the clock.
python scripts/gen_valu_probe11.py  (writes the .hip; build line in its header)"""
from gen_valu_probe9 import H_OPS, schedule
from gen_valu_probe10 import G, emit, inverse, runs

PERM_OF = 1  # the better of arms 1 and 2 in profiles/g_rotr16/probe.txt


def column_chain(k):
    """one G on column k with rotr16 as xor + alignbit, registers as gen_valu_probe9's (t unused)"""
    r = {n: f"v{8 + 7 * k + i}" for i, n in enumerate(("a", "b", "c", "d", "m0", "m1", "t"))}
    ops = [
        "v_add3_u32 {a}, {a}, {b}, {m0}",
        "v_xor_b32 {d}, {d}, {a}",
        "v_alignbit_b32 {d}, {d}, {d}, 16",
        "v_add_u32 {c}, {c}, {d}",
        "v_xor_b32 {b}, {b}, {c}",
        "v_alignbit_b32 {b}, {b}, {b}, 12",
        "v_add3_u32 {a}, {a}, {b}, {m1}",
        "v_xor_b32 {d}, {d}, {a}",
        "v_alignbit_b32 {d}, {d}, {d}, 8",
        "v_add_u32 {c}, {c}, {d}",
        "v_xor_b32 {b}, {b}, {c}",
        "v_alignbit_b32 {b}, {b}, {b}, 7",
    ]
    return [("H" if o.split()[0] in H_OPS else "F", o.format(**r)) for o in ops]


def inverse_keep16(lines):
    """as inverse(), but the F run in front of the rotate by 16 stays at priority 1"""
    rs = runs(lines)
    out = []
    for i, (c, body) in enumerate(rs):
        own = c == "F" and not rs[i + 1][1][0].endswith(", 16")  # the block ends in an H run
        out += (["s_setprio 0"] + body + ["s_setprio 1"]) if own else body
    return out


def with_perm(lines):
    return [ln.replace("v_alignbit_b32", "v_perm_b32").replace(", 16", ", %0") if ln.endswith(", 16") else ln
            for ln in lines]


P = schedule(4, "rr", chain=column_chain)
WINDOWED = {1: inverse(P), 2: inverse_keep16(P)}
ARMS = [
    ("control: SDWA rotr16, windows (H28 F20)", inverse(G), 1),
    ("xor + alignbit, xor in its own window", WINDOWED[1], 1),
    ("xor + alignbit, xor inside the H window", WINDOWED[2], 1),
    (f"arm {PERM_OF} with v_perm_b32 for the half swap", with_perm(WINDOWED[PERM_OF]), 1, '"s"(0x01000302u)'),
    ("xor + alignbit, no windows (H24 F24)", P, 0),
]

if __name__ == "__main__":
    emit(ARMS, "valu_probe11", "rotr16 as xor + alignbit under the priority windows over BLAKE3 G on gfx950",
         "profiles/g_rotr16/probe.txt", wps=(5, 6, 8))
