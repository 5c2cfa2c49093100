"""k_map's register and LDS budget, from the gfx950 code object's kernel descriptor (CPU only:
hipcc cross-compiles, as in tests/test_isa.py).

One 1024-thread workgroup per CU puts four waves on every SIMD, which leaves each wave 128 of the
SIMD's 512 VGPRs: a k_map that needs more does not launch.  Its LDS image is sized so that the key
tables fill what the staging, the lists and the letter table leave of the CU's 160 KiB; work on the
per-step code (the carried tokens are registers, not LDS) must not move it, because every byte
comes out of the tables' hit rate."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mit-6.824-2015_amd", "csrc", "wcg_api.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KMAPS = ["_ZN3wcg5k_mapILi0ELb1EEEvNS_7MapArgsE", "_ZN3wcg5k_mapILi0ELb0EEEvNS_7MapArgsE"]

VGPR_MAX = 128
# k_map's __shared__ arrays (wcg_map.h), in bytes:
#   wbytes   16 waves x 1032 staging bytes                   16512
#   wstart   16 waves x 512 u16 start-list entries           16384
#   wmask    16 waves x 64 u16 chunk masks                    2048
#   sk0      8410 short-key slots x 8                        67280
#   scnt     8410 x 4                                        33640
#   mk0, mk1 1024 medium-key slots x 8, twice                16384
#   mcnt     1024 x 4                                         4096
#   zero_w   8, seen_w (16384 admission bits) 2048            2056
#   cursor   128 miss buckets x 4, lcur 4                      516
#   lt_idx   0x314 + 4 letter-table block ids                  792
#   lt_bits  111 blocks x 8 words x 4                         3552
#   wsum     16 waves x 4 u64 stats                            512
#   alignment padding                                            4
LDS_BYTES = (16512 + 16384 + 2048 + 67280 + 33640 + 16384 + 4096 + 2056 + 516 + 792 + 3552 + 512 + 4)
assert LDS_BYTES == 163776      # the value in the descriptor before the carried tokens went raw


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_budget") / "wcg_api.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                        "-S", SRC, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def descriptor(asm, sym):
    m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, sym
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s*$", m.group(1), re.M)}


@pytest.mark.parametrize("kmap", KMAPS)
def test_map_vgpr_budget(device_asm, kmap):
    d = descriptor(device_asm, kmap)
    print(f"{kmap}: next_free_vgpr {d['next_free_vgpr']}")
    assert d["next_free_vgpr"] <= VGPR_MAX


@pytest.mark.parametrize("kmap", KMAPS)
def test_map_lds_size(device_asm, kmap):
    d = descriptor(device_asm, kmap)
    assert d["group_segment_fixed_size"] == LDS_BYTES
