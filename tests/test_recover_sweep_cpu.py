"""What the case generators of tests/test_gpu_recover_sweep.py and
tests/test_gpu_fuzz_recover.py reach, from their presence maps and case plans
alone (no oracle, no GPU): a later edit of the generators cannot silently empty
the GPU tests."""
import pytest

import test_gpu_fuzz_recover as fz
import test_gpu_recover_sweep as sw


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("ratio", sw.RATIOS)
@pytest.mark.parametrize("k", sw.KS)
def test_row_group_shapes_reach_every_class_in_both_halves(k, ratio, tail):
    n = ratio * k
    wn = sw.group_tail(n, k) if tail else n
    assert k < wn <= n and (wn % 16 == 8) == tail and (wn + k - 1) // k == ratio
    layouts = sw.group_layouts(n, k, wn)
    assert len(layouts) == 9 and [int(pr.sum()) for _, pr, _ in layouts[6:8]] == [k - 1, k]
    for count in (8, 9):
        pairs, words, cut, seg0 = sw.group_reach(layouts[:count], k, wn)
        print(f"n{n} k{k} wanted_n {wn} batch {count}: {len(pairs)} (class, half) pairs, {len(cut)} classes of the cut "
              f"group, {len(words)} (lower, upper) pairs of one row word")
        assert pairs >= {(c, h) for c in sw.CLASSES for h in (0, 1)}
        assert {("all-store", "all-compare"), ("all-compare", "all-store")} <= words
        assert seg0 == {False, True}
        assert cut >= set(sw.CLASSES) if tail else not cut
    # each class payload alters a present row beside a stored one, and a second present parity row
    for name, pres, flips in layouts:
        if flips is None:
            continue
        assert len(set(flips)) == 2 and all(pres[v] and k <= v < wn for v in flips)
        v = flips[0]
        beside = [u for u in (v - 1, v + 1) if u // 16 == v // 16 and u < wn]
        assert any(not pres[u] for u in beside), name
        if wn < n and int(name.split("-")[1]) % 2:
            assert 0 < int(pres[wn:].sum()) < n - wn  # random presence at and above wanted_n


def test_edge_and_wide_layouts():
    for n, k, wn in sw.EDGES:
        lay = sw.edge_layouts(n, k, wn)
        assert [int(pr.sum()) for _, pr, _ in lay[2:]] == [k, k - 1]
        assert int(lay[0][1].sum()) > k and lay[1][1][wn:].all() and int(lay[1][1].sum()) > k
        assert wn == 0 or (lay[0][1][:wn] == 0).any() and (lay[1][1][:wn] == 0).any()
        assert (len(lay[1][2]) == 1) == (wn > k)
        # a decodable payload with an absent row at or above wanted_n (a store there would show), and a present one
        assert wn == n or not lay[0][1][n - 1]
        assert wn >= n - 1 or lay[0][1][wn]
    edges = {wn for n, k, wn in sw.EDGES if (n, k) == (512, 64)}
    assert edges == {0, 1, 63, 64, 65, 79, 80, 81, 127, 128, 129, 511, 512}
    for n, k, wn, _ in sw.WIDE:
        sets = sw._wide_sets(n, k, wn)
        lay = sw.wide_layouts(n, k, wn, sets)
        assert len(lay) == len(sets) + 2
        for s, (name, pres, flips) in zip(sets, lay):
            absent = {int(v) // k for v in (pres[:wn] == 0).nonzero()[0]}
            assert absent == set(s) and len(flips) == 2 and all(pres[v] and k <= v < wn for v in flips), name
            assert pres[wn:].all() if s else not pres[wn:].any()
            stores = [v // k in absent for v in flips]
            if len(absent - {0}) and len(absent) < (wn + k - 1) // k - 1:
                assert stores == [True, False], name  # one in a segment that also stores, one in one that does not
        # segments 31, 32 and 33 take altered rows where the code has them
        if wn > 34 * k:
            assert {31, 32, 33} <= {v // k for _, _, flips in lay if flips for v in flips}


def test_fuzz_plans_cover_their_axes():
    plans = fz.all_plans()
    assert len(plans) == 24 + 20 and sum(pl.ragged for pl in plans) == 20
    uniform = [pl for pl in plans if not pl.ragged]
    assert {(pl.n, pl.k) for pl in uniform} == set(fz.SHAPES)
    assert {(pl.n, pl.k) for pl in plans if pl.ragged} == set(fz.RAGGED_DIRECT) | set(fz.RAGGED_WIDE)
    live = [max(1, (pl.wn + pl.k - 1) // pl.k) for pl in plans]
    assert 1 in live and 2 in live and any(lv == pl.n // pl.k for lv, pl in zip(live, plans))
    assert any(pl.wn % 16 for pl in plans)
    above = sum(any(int(pr[pl.wn:].sum()) for _, _, pr in pl.payloads) for pl in plans)
    both = sum(pl.combo[1] and pl.combo[2] for pl in plans)
    odd = sum(pl.odd_out for pl in plans)
    payloads = [(pl, pr) for pl in plans for _, _, pr in pl.payloads]
    decodable = sum(int(pr.sum()) >= pl.k for pl, pr in payloads)
    print(f"fuzz plans: {len(plans)} cases, {len(payloads)} payloads, {decodable} with >= k present rows "
          f"({decodable / len(payloads):.3f}); a present row at or above wanted_n in {above} cases; restore and "
          f"verify together in {both}; d_out at an odd address in {odd}; live segments {sorted(set(live))}; "
          f"requests {sorted({pl.combo for pl in plans})}")
    assert 3 * above >= len(plans) and 2 * both >= len(plans) and odd > 0
    assert any(pl.odd_out for pl in uniform) and any(pl.odd_out for pl in plans if pl.ragged)
    assert 3 * decodable >= 2 * len(payloads)
    assert len({pl.combo for pl in plans}) == 7
    for pl in plans:
        if pl.ragged:  # the placement: extents inside the buffers and disjoint, out of the batch's order somewhere
            spans = sorted((so, so + pl.n * sl) for _, _, so, sl in pl.items)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= pl.ssize
            outs = sorted((po, po + ln) for po, ln, _, _ in pl.items)
            assert all(a[1] <= b[0] for a, b in zip(outs, outs[1:])) and outs[-1][1] <= pl.psize
            assert all(so % 16 == 2 or so % 128 == 0 for _, _, so, _ in pl.items)
    assert any([it[2] for it in pl.items] != sorted(it[2] for it in pl.items) for pl in plans if pl.ragged)
