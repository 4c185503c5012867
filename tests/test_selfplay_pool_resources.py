"""The pool kernels' registers, from the compiler's remarks (no GPU): both float models of both kernels
exist in the selfplay namespace, none spills, and none has a lower occupancy than the
single-opponent kernel whose body it shares (the POOL switch changes the staging of P2's image, before the
tick loop, and nothing inside it)."""
import functools
import re

from tests.test_kernel_resources import kernel_resources

TWINS = {"k_step_n_selfplay_pool": "k_step_n_selfplay", "k_step_skip_pool_selfplay": "k_step_skip_selfplay"}


@functools.lru_cache(maxsize=None)
def _instances():
    out = {}
    for sym, r in kernel_resources("fs_kernels.hip").items():
        m = re.match(r"_ZN3fsk8selfplay\d+(k_step_\w+?)ILi(\d)EEE", sym)
        if m:
            out[(m.group(1), int(m.group(2)))] = r
    return out


def test_both_float_models_of_both_pool_kernels_exist():
    inst = _instances()
    assert sorted(inst) == sorted((k, fm) for pair in TWINS.items() for k in pair for fm in (0, 1)), sorted(inst)


def test_pool_kernels_keep_their_twins_resources():
    inst = _instances()
    for pool, twin in TWINS.items():
        for fm in (0, 1):
            p, t = inst[(pool, fm)], inst[(twin, fm)]
            assert p.get("ScratchSize", -1) == 0 and t.get("ScratchSize", -1) == 0, (pool, fm, p, t)
            assert p.get("Occupancy", 0) >= t.get("Occupancy", 0) >= 2, (pool, fm, p, t)
