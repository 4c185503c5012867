"""k_step_skip_selfplay's registers, from the compiler's remarks (no GPU): both float models exist,
neither spills, and two waves fit a SIMD -- 65 536 arenas are two waves per SIMD, i.e. at most 256
VGPRs, with both actors' weight fragments read from LDS and the per-arena counters in registers."""
import functools

from tests.test_kernel_resources import kernel_resources


@functools.lru_cache(maxsize=None)
def _instances():
    res = kernel_resources("fs_kernels.hip")
    return {k: v for k, v in res.items() if "k_step_skip_selfplay" in k}


def test_both_float_models_exist_in_the_selfplay_namespace():
    names = sorted(_instances())
    assert len(names) == 2, names
    for fm, name in enumerate(names):
        assert name.startswith("_ZN3fsk8selfplay20k_step_skip_selfplayILi%dEEE" % fm), name


def test_spill_free_at_two_waves_per_simd():
    inst = _instances()
    assert inst
    for name, r in inst.items():
        assert r.get("ScratchSize", -1) == 0, (name, r)
        assert r.get("Occupancy", 0) >= 2, (name, r)
