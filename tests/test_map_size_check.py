"""The host bound that lets k_map count its steps in 32 bits (wcg_map_size_check, CPU only).

k_map's step index, step count and stride are 32-bit so that their compares run on the scalar
unit.  A call has ceil(n / 992) steps, and a wave looks MAP_SETS strides (G * 16 steps each) past
its current step, so the library keeps the last 2^24 indices free: a call with more than
2^32 - 1 - 2^24 steps is WCG_EINVAL.  wcg_map_device applies the check before it looks at the
pointer or the device; here the check is called directly, so nothing touches a device."""
MAP_STEP = 992
STEPS_MAX = 0xFFFFFFFF - (1 << 24)


def test_size_check_bound(built):
    import wcg
    lib = wcg.load()
    ok, einval = 0, 1
    assert lib.wcg_map_size_check(0) == ok
    assert lib.wcg_map_size_check(1) == ok
    assert lib.wcg_map_size_check(1 << 40) == ok                        # 1 TiB
    assert lib.wcg_map_size_check(STEPS_MAX * MAP_STEP) == ok            # exactly the last step count
    assert lib.wcg_map_size_check(STEPS_MAX * MAP_STEP + 1) == einval    # one byte opens one more step
    assert lib.wcg_map_size_check((1 << 32) * MAP_STEP) == einval        # a step count past 32 bits
    assert lib.wcg_map_size_check((1 << 64) - 1) == einval               # no wrap in the rounding up
