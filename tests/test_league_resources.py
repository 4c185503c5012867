"""The league kernels' registers, from the compiler's remarks (no GPU): both float models of both kernels exist
in the league namespace, none uses scratch, and each keeps two waves per SIMD -- what 65 536 arenas are, and
what the two bodies of a kernel (a remote group's and a bot group's) must fit side by side."""
import functools
import re

from tests.test_kernel_resources import kernel_resources

KERNELS = ("k_step_n_league", "k_step_skip_league")


@functools.lru_cache(maxsize=None)
def _instances():
    out = {}
    for sym, r in kernel_resources("fs_kernels.hip").items():
        m = re.match(r"_ZN3fsk6league\d+(k_step_\w+?)ILi(\d)EEE", sym)
        if m:
            out[(m.group(1), int(m.group(2)))] = r
    return out


def test_both_float_models_of_both_league_kernels_exist():
    inst = _instances()
    assert sorted(inst) == sorted((k, fm) for k in KERNELS for fm in (0, 1)), sorted(inst)


def test_league_kernels_use_no_scratch_at_two_waves_per_simd():
    for key, r in _instances().items():
        assert r.get("ScratchSize", -1) == 0, (key, r)
        assert r.get("Occupancy", 0) >= 2, (key, r)
