"""tests/sampling_full_spec.py (whole-vocabulary sampling, integer masses) pinned to tests/sampling_spec.py (the top-k sampler's contract, fp32
sums in a fixed order): for V <= 512 and top_k = V the older specification keeps every token as a candidate, so both describe the same
warpers and the same draw, and they must agree wherever the older one's own margins say that its fp32 rounding cannot matter."""
import numpy as np

import sampling_full_spec as full
import sampling_spec as spec

MARGIN = 1e-5


def test_integer_masses_are_exact_and_the_limit_is_a_floor():
    e = np.array([1.0, 0.5, 2.0 ** -32, 2.0 ** -33, 0.0, np.float32(0.3)], dtype=np.float32)
    q = full.quantise(e)
    assert q.dtype == np.uint64 and q.tolist() == [1 << 32, 1 << 31, 1, 0, 0, int(float(np.float32(0.3)) * 2 ** 32)]
    for top_p in (0.95, 0.3, 1e-6, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))):
        for Q in (1 << 32, 217_488 << 32, 123_456_789_012_345):
            from fractions import Fraction
            assert full.top_p_limit(top_p, Q) == int(Fraction(float(np.float32(top_p))) * Q)      # (Fraction of a float is exact; int() floors)


def test_agrees_with_the_topk_specification_at_top_k_equal_v():
    """180 seeded cases (V = 64 / 300 / 512, the sigma / T / top_p / min_p grid of sampling_spec.case_rows, one step, seeds 5 + i): the same
    survivors and the same token wherever the older specification's cut_margin and margin exceed its MARGIN."""
    compared = 0
    for i, (x, _, T, top_p, min_p) in enumerate(spec.case_rows(5, plan=((64, 60), (300, 60), (512, 60)))):
        V = x.size
        old = spec.sample(x, V, T, 5 + i, 0, top_p, min_p)
        new = full.sample(x, T, 5 + i, 0, top_p, min_p)
        if old.cut_margin > MARGIN:
            assert np.array_equal(np.flatnonzero(new.keep), old.ids), (i, V, T, top_p, min_p)
            if old.margin > MARGIN:
                assert new.token == old.token, (i, V, T, top_p, min_p, new.token, old.token, old.margin)
                compared += 1
    assert i == 179 and compared >= 170, compared


def test_windows_nest_and_the_draw_is_a_function_of_the_row():
    rng = np.random.default_rng(3)
    x = spec.bf16_round(rng.standard_normal(1003).astype(np.float32) * 2)
    strict = full.survivors(x, 0.9, 0.8, 0.01, delta=-MARGIN)
    exact = full.survivors(x, 0.9, 0.8, 0.01)
    loose = full.survivors(x, 0.9, 0.8, 0.01, delta=+MARGIN)
    assert not (strict & ~exact).any() and not (exact & ~loose).any() and 1 <= exact.sum() < x.size
    d = full.sample(x, 0.9, 11, 4, 0.8, 0.01)
    assert full.token_in_window(d, d.token) and d.keep[d.token] and d.S == int(d.q[d.keep].sum(dtype=np.uint64))
    perm = rng.permutation(x.size)                       # the masses are integers: any order of summation gives S
    assert int(d.q[d.keep][rng.permutation(int(d.keep.sum()))].sum(dtype=np.uint64)) == d.S and perm.size == x.size
    words = np.zeros((x.size + 31) // 32, dtype=np.uint32)
    for c in np.flatnonzero(d.keep):
        words[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    assert np.array_equal(full.bits_to_mask(words, x.size), d.keep)
