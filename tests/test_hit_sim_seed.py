"""CPU: the simulated hit rate of k_map's seeded LDS tables for the shipped SEED_FRAC.

DESIGN.md section 22 chooses SEED_FRAC from tools/hit_sim.py's table and compares the GPU's measured
lds_hits / tokens with the simulator's figure for it; this reproduces that figure (the generator,
the regular expression and the simulator's hashes are deterministic), so a change to the simulator,
the corpus or the constant shows up here.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMULATED = {(3, 4): 0.7786}     # SEED_NUM / SEED_DEN -> the figure of DESIGN.md section 22


def shipped_frac():
    text = open(os.path.join(ROOT, "mit-6.824-2015_amd", "csrc", "wcg_seed.h")).read()
    m = re.search(r"constexpr u32 SEED_NUM = (\d+), SEED_DEN = (\d+);", text)
    assert m, "wcg_seed.h no longer spells SEED_NUM / SEED_DEN this way"
    return int(m.group(1)), int(m.group(2))


def test_simulated_rate_of_the_shipped_seed_frac(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hit_sim
    num, den = shipped_frac()
    assert (num, den) in SIMULATED, "a new SEED_FRAC needs its simulated figure here and in DESIGN.md"
    rate = hit_sim.seeded_rate(num / den)
    print(f"simulated hit rate, {num}/{den} of the slots offered: {rate:.4f}")
    assert abs(rate - SIMULATED[(num, den)]) <= 0.002
