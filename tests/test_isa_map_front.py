"""k_map's all-ASCII front end and start-list slots in the gfx950 assembly (CPU only:
hipcc cross-compiles, as in tests/test_isa_map_scalar.py).

k_map is VALU-issue bound (DESIGN.md sections 17-19), so what its per-step code costs shows in the
number of vector instructions the compiler emits for it.  For both k_map<0, *> instances this counts
the instruction lines that start with `v_` in the kernel's body (every process() copy of the
unrolled main loop, the tail loop and the drain: a static count, not a per-step one) and bounds it
by the value that section 19's changes reached, with the parent's value beside it:

  the 16 letter flags gathered by v_dot4_u32_u8, the neighbour masks shifted by DPP with bound_ctrl
  (no zeroing move in front of each), no rune-carry merge on the step's common path, and the
  short slots' run length from the window inverted once per step.

The bound must also stay strictly below the parent's value.  The registers, the LDS image and the
scratch size are the parent's (tests/test_isa_map_budget.py holds their limits; here they must not
have moved at all)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mit-6.824-2015_amd", "csrc", "wcg_api.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

#                                                   bound  parent
VALU_LINES = {"_ZN3wcg5k_mapILi0ELb1EEEvNS_7MapArgsE": (6212, 6302),     # split miss buckets (one-pass jobs)
              "_ZN3wcg5k_mapILi0ELb0EEEvNS_7MapArgsE": (6202, 6292)}     # mixed buckets (two-pass jobs)
NEXT_FREE_VGPR = 97
LDS_BYTES = 163776
SCRATCH_BYTES = 0


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_front") / "wcg_api.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                        "-S", SRC, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def body(asm, sym):
    """the kernel's instructions (no labels, directives or comment lines)"""
    m = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert m, sym
    lines = [ln.strip() for ln in m.group(1).split("\n")]
    return [ln for ln in lines if ln and not ln.startswith((";", ".")) and not ln.endswith(":")]


def descriptor(asm, sym):
    m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, sym
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s*$", m.group(1), re.M)}


@pytest.mark.parametrize("kmap", list(VALU_LINES))
def test_map_static_valu(device_asm, kmap):
    bound, parent = VALU_LINES[kmap]
    got = sum(ln.startswith("v_") for ln in body(device_asm, kmap))
    print(f"{kmap}: {got} VALU lines (bound {bound}, parent {parent})")
    assert bound < parent
    assert got <= bound


@pytest.mark.parametrize("kmap", list(VALU_LINES))
def test_map_letter_flags_by_dot4(device_asm, kmap):
    ins = body(device_asm, kmap)
    n = sum(ln.startswith("v_dot4_u32_u8") for ln in ins)
    print(f"{kmap}: {n} v_dot4_u32_u8")
    assert n >= 4                                   # four per ascii_mask16


@pytest.mark.parametrize("kmap", list(VALU_LINES))
def test_map_budget_unchanged(device_asm, kmap):
    d = descriptor(device_asm, kmap)
    print(f"{kmap}: next_free_vgpr {d['next_free_vgpr']}, LDS {d['group_segment_fixed_size']}, "
          f"scratch {d['private_segment_fixed_size']}")
    assert d["next_free_vgpr"] == NEXT_FREE_VGPR
    assert d["group_segment_fixed_size"] == LDS_BYTES
    assert d["private_segment_fixed_size"] == SCRATCH_BYTES
