"""Trajectory stores at byte offsets with the top bit set, and the real launch split of fs_step_n_packed.

The fused kernels store each trajectory row at base + a uint32 byte offset (st_off, csrc/fs_kernels.hip) and
fs_api.cpp splits a call so that the offsets fit: (2^32 - 1) / 32 rows per packed launch.  These are the smallest
shapes at which that arithmetic can go wrong -- large in bytes, not in time; one sign-extended offset would be a
write 4 GiB below the buffer:

A   fs_step_n_packed, 65 536 arenas, remote P2, same-step, 2049 ticks: the lane offsets pass 2^31 from tick 1024 and
    the call runs as launches of 2047 and 2 ticks, FOOTSIES_MAX_LAUNCH_ROWS unset (launch 1's last lane offset is
    32 (2047 * 65536 - 1) + 16 = 4 292 870 128).  72 B a row, 9.7 GB.
A'  the same on a next-step handle (the generic loop, no final_lanes): 40 B a row, 5.4 GB.
B   fs_step_n over action rows, next-step, 4100 ticks: row 2^28 is tick 4096, where the 8-byte-a-row fields reward,
    position and move_frame pass offset 2^31.  38 B a row, 10.2 GB.

Every row is checked on the device: the big arrays, 0xFF-filled with GUARD_ROWS guard rows behind each, against the
same action rows run on a second handle in launches of 512 ticks (at most 1000: the shape test_gpu_bench_shapes
holds to the oracle) into a small 0xFF-filled buffer, range by range on the byte views -- final_lanes of arenas that
did not end included: still 0xFF -- and both final states.  Independently of any kernel, three oracles of 256
arenas (arena_base 0, 32 640, 65 280; arenas do not interact) step their columns of the rows for all ticks and are
compared with the big trajectory at tick 0, the ticks around every 2^31 crossing of every record size, the ticks
around the launch split, the last tick and every 97th, and with the handle's state at the end."""
import os
import time

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import compare_outputs, compare_states, fused_kernel
from tests.test_gpu_bench_shapes import KERNEL

pytestmark = pytest.mark.gpu

N = 65536
SEED, SIM_SEED = 0x5EED, 11
GUARD_ROWS = 4096
CHUNK = 512          # ticks per launch of the second handle
ORACLE_BASES = (0, 32640, 65280)
ORACLE_N = 256
EVERY = 97
PACKED_ROWS = (2**32 - 1) // 32  # fs_api.cpp kMaxPackedLaunchRows: 2^27 - 1
TORCH = {"u1": "uint8", "f4": "float32", "f8": "float64", "i4": "int32"}


def packed_fields(same_step):
    """name -> bytes per row"""
    return {"lanes": 32, "reward": 8, **({"final_lanes": 32} if same_step else {})}


def per_field_fields(same_step):
    return {k: np.dtype(dt).itemsize * cols for k, (dt, cols) in _abi.OUTPUT_SPEC.items()
            if same_step or not k.startswith("final_")}


def crossings(fields, launches):
    """The ticks (t - 1, t) of the call where a record's byte offset within its launch first reaches a multiple
    of 2^31: row k 2^31 / size of the launch."""
    out, first = set(), 0
    for m in launches:
        for size in set(fields.values()):
            t, rest = divmod(2**31 // size, N)  # (sizes are powers of two; 2 * 2^31 is past every offset)
            if t < m:
                assert rest == 0 and t > 0
                out |= {first + t - 1, first + t}
        first += m
    return out


def compared_ticks(n, fields, launches):
    ticks = {0, n - 1} | set(range(0, n, EVERY)) | crossings(fields, launches)
    for at in np.cumsum(launches)[:-1]:
        ticks |= {int(at) - 1, int(at)}
    return sorted(ticks)


class Arrays:
    """One 0xFF-filled uint8 device buffer per field, `ticks` x N rows and GUARD_ROWS more."""

    def __init__(self, fields, ticks, guard, dev):
        import torch
        self.fields, self.rows, self.guard = fields, ticks * N, guard
        self.raw = {k: torch.full(((self.rows + guard) * size,), 0xFF, dtype=torch.uint8, device=dev)
                    for k, size in fields.items()}

    def refill(self):
        for t in self.raw.values():
            t.fill_(0xFF)

    def typed(self, packed):
        """The tensors a step call takes."""
        import torch
        if packed:
            return {"lanes": self.raw["lanes"], "reward": self.raw["reward"].view(torch.float64),
                    "final_lanes": self.raw.get("final_lanes")}
        return {k: t.view(getattr(torch, TORCH[_abi.OUTPUT_SPEC[k][0]])) for k, t in self.raw.items()}

    def span(self, k, tick0, ticks):
        size = self.fields[k]
        return self.raw[k][tick0 * N * size:(tick0 + ticks) * N * size]

    def guard_untouched(self):
        return all(bool((t[self.rows * self.fields[k]:] == 0xFF).all()) for k, t in self.raw.items())

    def host_rows(self, packed, tick, a0, a1):
        """Tick `tick`'s outputs of arenas a0 .. a1 - 1 as numpy fields."""
        from footsies_gym_amd.simulator import unpack_trajectory
        rec = {}
        for k, size in self.fields.items():
            rec[k] = self.raw[k][(tick * N + a0) * size:(tick * N + a1) * size].cpu().numpy()
        if packed:
            rec = {k: (v.reshape(a1 - a0, 2, 16) if k != "reward" else v.view(np.float64)) for k, v in rec.items()}
            rec.setdefault("final_lanes", None)
            return {k: np.ascontiguousarray(v) for k, v in unpack_trajectory(rec).items()}
        out = {}
        for k, v in rec.items():
            dt, cols = _abi.OUTPUT_SPEC[k]
            out[k] = v.view(dt).reshape((a1 - a0, cols) if cols > 1 else (a1 - a0,))
        return out


def oracle_rows(oracle_lib, same_step, h1, h2, ticks):
    """The three oracles over their columns of the action rows (host [n][N]): {tick: [outputs per oracle]} for
    `ticks`, and the oracles (at the end of the run)."""
    oras = [oracle_lib.Oracle(ORACLE_N, p2_mode=_abi.FS_P2_EXTERNAL, base_seed=SIM_SEED, arena_base=b,
                              autoreset_mode=_abi.FS_AUTORESET_SAME_STEP if same_step else _abi.FS_AUTORESET_NEXT_STEP)
            for b in ORACLE_BASES]
    cols = [(np.ascontiguousarray(h1[:, b:b + ORACLE_N]), np.ascontiguousarray(h2[:, b:b + ORACLE_N])) for b in ORACLE_BASES]
    want, out = set(ticks), {}
    for t in range(len(h1)):
        rows = [o.step(c1[t], c2[t]) for o, (c1, c2) in zip(oras, cols)]
        if t in want:
            out[t] = rows
    return out, oras


def rounds_end_on_both_sides(exp, ticks, crossing):
    """From the oracle alone: some compared tick before the first 2^31 crossing ends a round, and some at or
    after it."""
    ended = {t: any(r["terminated"].any() for r in exp[t]) for t in ticks}
    return any(v for t, v in ended.items() if t < crossing), any(v for t, v in ended.items() if t >= crossing)


CASES = {
    "A-packed-same_step-2049": dict(packed=True, same_step=True, n=2049, split=True),
    "A'-packed-next_step-2049": dict(packed=True, same_step=False, n=2049, split=True),
    "B-per_field-next_step-4100": dict(packed=False, same_step=False, n=4100, split=False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_offsets_past_2_31(oracle_lib, name):
    import torch
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim
    case = CASES[name]
    packed, same_step, n = case["packed"], case["same_step"], case["n"]
    assert "FOOTSIES_MAX_LAUNCH_ROWS" not in os.environ  # the library's own limits
    fields = packed_fields(same_step) if packed else per_field_fields(same_step)
    row_bytes = sum(fields.values())
    assert row_bytes == {"A-": 72, "A'": 40, "B-": 38}[name[:2]]
    launches = [2047, 2] if case["split"] else [n]
    if case["split"]:
        assert 2047 == (2**27 - 1) // N == PACKED_ROWS // N and 32 * (2047 * N - 1) + 16 == 4292870128 < 2**32
    else:
        assert n * N <= (2**32 - 1) // 8  # one launch
    ticks = compared_ticks(n, fields, launches)
    cross = sorted(crossings(fields, launches))
    assert cross == ([1023, 1024] if packed else [4095, 4096]), cross
    if case["split"]:
        assert {2046, 2047, 2048} <= set(ticks)

    need = (n * N + GUARD_ROWS) * row_bytes + (CHUNK * N + GUARD_ROWS) * row_bytes + 2 * n * N
    free, total = torch.cuda.mem_get_info()
    if free < need + 2 * 2**30:
        pytest.skip("%s needs %d bytes + 2 GiB of device memory, %d are free" % (name, need, free))
    dev = torch.device("cuda", 0)
    torch.cuda.reset_peak_memory_stats()
    t_start = time.perf_counter()
    mode = "same_step" if same_step else "next_step"
    sim = FootsiesSim(N, p2_mode="external", autoreset_mode=mode, seed=SIM_SEED)
    if name.startswith("A-"):  # the headline kernel
        kname = lib().fs_step_kernel(sim.handle, launches[0], _abi.FS_KERNEL_PACKED).decode()
        assert kname == fused_kernel(KERNEL["external"], N) or os.environ.get("FOOTSIES_FUSED_LANES") == "1", kname
    p1, p2 = sim.hash_actions(n, seed=SEED)
    big = Arrays(fields, n, GUARD_ROWS, dev)
    if packed:
        sim.step_n_packed(n, p1, p2, trajectory=big.typed(True))
    else:
        sim.step_n(n, p1, p2, trajectory=big.typed(False))
    torch.cuda.synchronize()
    assert sim.steps_taken == n
    assert big.guard_untouched(), "a store landed behind the last row"

    # every row against the second handle's launches of CHUNK ticks
    twin = FootsiesSim(N, p2_mode="external", autoreset_mode=mode, seed=SIM_SEED)
    small = Arrays(fields, CHUNK, GUARD_ROWS, dev)
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        small.refill()
        if packed:
            twin.step_n_packed(m, p1[k:k + m], p2[k:k + m], trajectory=small.typed(True))
        else:
            twin.step_n(m, p1[k:k + m], p2[k:k + m], trajectory=small.typed(False))
        torch.cuda.synchronize()
        for f in fields:
            assert torch.equal(big.span(f, k, m), small.span(f, 0, m)), "%s differs in ticks %d .. %d" % (f, k, k + m - 1)
        assert small.guard_untouched()
    state = sim.get_state()
    compare_states(twin.get_state(), state)
    twin.close()
    del small, twin

    # the oracle, independently of any kernel
    h1, h2 = p1.cpu().numpy(), p2.cpu().numpy()
    exp, oras = oracle_rows(oracle_lib, same_step, h1, h2, ticks)
    for t in ticks:
        for b, rows in zip(ORACLE_BASES, exp[t]):
            compare_outputs(rows, big.host_rows(packed, t, b, b + ORACLE_N), step=t, same_step=same_step)
    for b, o in zip(ORACLE_BASES, oras):
        compare_states(o.state(), state[b:b + ORACLE_N])
        o.close()
    before, after = rounds_end_on_both_sides(exp, ticks, cross[1])
    assert before and after, "no round ended in the compared ticks %s the 2^31 crossing" % ("before" if after else "past")
    peak = torch.cuda.max_memory_allocated()
    print("%s: %d rows x %d B, %d ticks compared with the oracle, peak device memory %.2f GB, %.1f s" % (
        name, n * N, row_bytes, len(ticks), peak / 1e9, time.perf_counter() - t_start))
    sim.close()
    del big, sim, p1, p2
    torch.cuda.empty_cache()
