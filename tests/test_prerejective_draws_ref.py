"""tests/prerejective_draws_ref.py (the tile scheme of the device draws in Python integers) against tests/prerejective_ref.draws,
the serial loop: jump-ahead, the tables, their composition, the emission, the budget rule and both fallback words.  No GPU."""
import numpy as np
import pytest

import prerejective_draws_ref as dref
import prerejective_ref as ref

SHAPES = [(634, 3, 5, 2000, 1), (3, 3, 1, 300, 7), (8, 8, 8, 300, 9), (9, 8, 2, 300, 9), (4096, 3, 8, 1000, 2 ** 63 + 5)]
IDS = ["-".join(str(v) for v in s[:4]) for s in SHAPES]


@pytest.fixture(scope="module")
def tiled():
    return {s: dref.draws_tiled(*s) for s in SHAPES}


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5, 2 ** 64 - 1])
def test_jump_ahead_equals_stepping(seed):
    want, x, at = {}, seed, 0
    for p in sorted([0, 1, 2, 63, 64, 4097]):
        while at < p:
            x, at = dref.step(x), at + 1
        want[p] = x
    for p, v in want.items():
        assert dref.state_at(seed, p) == v, p
    # 2^20 + 3: from the jumped 2^20 (itself 2^10 jumps of 2^10 stepped once), three steps
    a, c = 1, 0
    for _ in range(1 << 10):
        a, c = (a * dref.A) & dref.MASK, (c * dref.A + dref.C) & dref.MASK
    x = seed
    for _ in range(1 << 10):
        x = (x * a + c) & dref.MASK
    for _ in range(3):
        x = dref.step(x)
    assert dref.state_at(seed, (1 << 20) + 3) == x


def test_jump_table_is_repeated_squaring():
    x = 12345
    for k, (a, c) in enumerate(dref.JUMP[:12]):
        y = x
        for _ in range(1 << k):
            y = dref.step(y)
        assert (x * a + c) & dref.MASK == y, k


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tiles_compose_to_the_serial_draws(tiled, shape):
    ns, S, K, H, seed = shape
    samp, pick = ref.draws(ns, S, K, H, seed)
    got = tiled[shape]
    assert got["word"] == 0
    np.testing.assert_array_equal(got["samples"], samp)
    np.testing.assert_array_equal(got["picks"], pick)
    starts = dref.iteration_starts(ns, S, K, H, seed)
    assert got["starts"] == starts[:-1] and got["consumed"] == starts[-1]
    print(f"{shape[:4]}: P {got['P']}, consumed {got['consumed']}, longest iteration {got['longest']}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_budget_covers_the_consumed_positions(tiled, shape):
    ns, S, K, H, seed = shape
    assert dref.budget(ns, S, H) == tiled[shape]["P"] >= dref.iteration_starts(ns, S, K, H, seed)[-1]


def test_longest_iterations_of_the_issue():
    assert max(np.diff(dref.iteration_starts(634, 3, 5, 2000, 1))) == 7
    assert max(np.diff(dref.iteration_starts(8, 8, 8, 300, 9))) == 84


def test_small_tiles_and_windows_give_the_same_draws():
    ns, S, K, H, seed = 9, 8, 2, 300, 9
    samp, pick = ref.draws(ns, S, K, H, seed)
    for T, W in ((256, 64), (512, 256)):
        longest = max(np.diff(dref.iteration_starts(ns, S, K, H, seed)))
        got = dref.draws_tiled(ns, S, K, H, seed, window=W, T=T)
        if longest <= W:
            assert got["word"] == 0
            np.testing.assert_array_equal(got["samples"], samp)
            np.testing.assert_array_equal(got["picks"], pick)
        else:
            assert got["word"] == dref.OVERFLOW


def test_a_window_of_24_overflows():
    got = dref.draws_tiled(8, 8, 8, 300, 9, window=24)
    assert got["word"] == dref.OVERFLOW
    # what was emitted before the iteration that did not fit is still the serial loop's
    samp, _ = ref.draws(8, 8, 8, 300, 9)
    done = int((got["samples"][:, 0] >= 0).sum())
    lens = np.diff(dref.iteration_starts(8, 8, 8, 300, 9))
    assert done == int(np.argmax(lens > 24)) < 300           # everything before the first iteration that does not fit
    np.testing.assert_array_equal(got["samples"][:done], samp[:done])


def test_a_budget_of_2SH_is_short():
    got = dref.draws_tiled(3, 3, 1, 300, 7, budget_positions=2 * 3 * 300)
    assert got["word"] == dref.SHORT
    starts = dref.iteration_starts(3, 3, 1, 300, 7)
    done = int((got["samples"][:, 0] >= 0).sum())
    assert done == sum(1 for p in starts[:-1] if p < 1800) < 300
