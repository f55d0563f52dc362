"""The tile scheme of prerejective_draws.hip restated with Python integers: the LCG's jump-ahead, the length of the iteration that
would start at every stream position, the per-tile exit tables, their composition in order and the emission of the iterations
that really start, with the overflow and short words and the stream budget.  DESIGN.md 4.26 has the argument.

Nothing here calls the library.  test_prerejective_draws_ref.py pins this file against prerejective_ref.draws."""
import math

import numpy as np

MASK = 0xFFFFFFFFFFFFFFFF
A, C = 6364136223846793005, 1442695040888963407
TILE, WINDOW = 1024, 256
OVERFLOW, SHORT = 1, 2
NO_ENTRY = None


def step(x):
    return (x * A + C) & MASK


def unit(x):
    return float(x >> 11) * (1.0 / 9007199254740992.0)


def jump_table(bits=32):
    """(a_k, c_k): x -> a_k x + c_k is 2^k steps."""
    out, a, c = [], A, C
    for _ in range(bits):
        out.append((a, c))
        a, c = (a * a) & MASK, (c * (a + 1)) & MASK
    return out


JUMP = jump_table()


def state_at(seed, p):
    """The state after p steps from the seed, by the set bits of p."""
    x = int(seed) & MASK
    for k, (a, c) in enumerate(JUMP):
        if (p >> k) & 1:
            x = (x * a + c) & MASK
    assert p >> len(JUMP) == 0
    return x


def iteration(x, ns, S, K, W):
    """The iteration that starts at state x: (length in positions or 0 when it needs more than W, samples, picks)."""
    got, used = [], 0
    while len(got) < S and used < W - S:
        x = step(x)
        used += 1
        si = int(ns * unit(x))
        if si not in got:
            got.append(si)
    if len(got) < S:
        return 0, None, None
    picks = []
    for _ in range(S):
        x = step(x)
        picks.append(int(K * unit(x)))
    return used + S, got, picks


def budget(ns, S, H, W=WINDOW):
    """P = ceil(H (2 S + E) + 8 sqrt(H V) + W) in float64."""
    E = V = 0.0
    for j in range(S):
        q = j / ns
        E += ns / (ns - j) - 1.0
        V += q / ((1.0 - q) * (1.0 - q))
    return int(math.ceil(H * (2.0 * S + E) + 8.0 * math.sqrt(H * V) + W))


def tile_lengths(seed, tile, ns, S, K, W, T=TILE):
    """len of the T positions of a tile, each from its own jump (kernels A and C)."""
    return [iteration(state_at(seed, tile * T + o), ns, S, K, W)[0] for o in range(T)]


def tile_table(lens, end, W, T=TILE):
    """Kernel A: per entry offset e < W (exit offset into the next tile, iterations started below `end`, stuck on a len of 0)."""
    rows = []
    for e in range(W):
        off, cnt, stuck = e, 0, False
        while off < end:
            l = lens[off]
            if l == 0:
                stuck = True
                break
            off += l
            cnt += 1
        rows.append((off - T if off >= T else 0, cnt, stuck))
    return rows


def compose(tables, H):
    """Kernel B: every tile's (true entry or NO_ENTRY, first iteration), and the problem's word."""
    entries, e, it, word = [], 0, 0, 0
    for rows in tables:
        live = e is not NO_ENTRY and it < H
        entries.append((e if live else NO_ENTRY, it))
        if not live:
            e = NO_ENTRY
            continue
        ex, cnt, stuck = rows[e]
        it += cnt
        if stuck and it < H:
            word |= OVERFLOW
            e = NO_ENTRY
            continue
        e = ex
    if not word & OVERFLOW and it < H:
        word |= SHORT
    return entries, word


def draws_tiled(ns, S, K, H, seed, window=0, budget_positions=0, T=TILE):
    """The whole scheme for one problem: dict(samples, picks (H, S) int32, rows never emitted stay -1; word; P; consumed = the
    position after the last emitted iteration; longest = the longest emitted iteration; starts = position of every emitted one)."""
    W = window or WINDOW
    P = budget_positions or budget(ns, S, H, W)
    tiles = (P + T - 1) // T
    lens = [tile_lengths(seed, t, ns, S, K, W, T) for t in range(tiles)]
    tables = [tile_table(lens[t], min(T, P - t * T), W, T) for t in range(tiles)]
    entries, word = compose(tables, H)
    samples, picks = np.full((H, S), -1, np.int32), np.full((H, S), -1, np.int32)
    starts, consumed, longest = [], 0, 0
    for t, (e, first) in enumerate(entries):           # kernel C
        if e is NO_ENTRY:
            continue
        off, k, end = e, 0, min(T, P - t * T)
        while off < end and first + k < H:
            if lens[t][off] == 0:
                break
            n, sm, pk = iteration(state_at(seed, t * T + off), ns, S, K, W)
            assert n == lens[t][off]
            samples[first + k], picks[first + k] = sm, pk
            starts.append(t * T + off)
            off += n
            k += 1
            consumed, longest = t * T + off, max(longest, n)
    return dict(samples=samples, picks=picks, word=word, P=P, consumed=consumed, longest=longest, starts=starts)


def iteration_starts(ns, S, K, H, seed):
    """The stream position at which every iteration of the serial loop (prerejective_ref.draws) starts, and the position after the
    last: H + 1 values."""
    x, pos, out = int(seed) & MASK, 0, []
    for _ in range(H):
        out.append(pos)
        got = []
        while len(got) < S:
            x = step(x)
            pos += 1
            si = int(ns * unit(x))
            if si not in got:
                got.append(si)
        for _ in range(S):
            x = step(x)
            pos += 1
    out.append(pos)
    return out
