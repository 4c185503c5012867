"""k_step_n_selfplay's registers, from the compiler's remarks (no GPU): 65 536 arenas are two waves
per SIMD, so every instance has to fit two (P1's weight fragments in registers, P2's read from LDS
every tick) and none may spill."""
import re

from tests.test_kernel_resources import kernel_resources


def test_selfplay_kernels_fit_two_waves_per_simd_without_scratch():
    # fsk::selfplay::k_step_n_selfplay<FM>
    res = {k: v for k, v in kernel_resources("fs_kernels.hip").items() if re.search(r"\b_ZN3fsk8selfplay\d+k_step_n_selfplayI", k)}
    assert sorted(re.search(r"k_step_n_selfplayILi(\d)E", k).group(1) for k in res) == ["0", "1"], sorted(res)  # both float models
    for k, v in res.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
