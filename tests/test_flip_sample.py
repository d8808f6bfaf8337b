"""tests/flip_sweep.py select_cells -- the pure sample selection of the layout sweep (tests/test_gpu_flip_layouts.py) --
on hand-written layouts: sections with 0, 1 and 2 jumps, a jump exactly at a section's first cell, a one-cell section."""
from tests.flip_sweep import FREE_PROLOGUE, free_epilogue, select_cells


def sec(name, cells, jumps=(), free=(), zero=None, lookups=0, limb_calls=0):
    return dict(name=name, cells=cells, jumps=list(jumps), free=list(free), zero=zero, lookups=lookups, limb_calls=limb_calls)


def context(target0, target1):
    """Two digests.  Digest 0: a prologue with the zero cell behind it and one jump inside; a block with two jumps, the
    second one cell before its end; a block without; an epilogue whose last cell is followed by a jump.  Digest 1: that
    jump seen from the other side -- exactly at the prologue's first cell; a one-cell section; an epilogue with a jump
    behind its first cell."""
    return [[sec("prologue", 101, [40], free=[FREE_PROLOGUE], zero=100, lookups=7),
             sec("block0", 500, [17, 499], lookups=30, limb_calls=40),
             sec("block1", 500, lookups=30, limb_calls=40),
             sec("epilogue", 76 * 3 + 288, [76 * 3 + 288], free=[free_epilogue(target0)], lookups=64)],
            [sec("prologue", 60, [0], free=[FREE_PROLOGUE], lookups=5),
             sec("block0", 1, lookups=1, limb_calls=1),
             sec("epilogue", 76 * 2 + 288, [1], free=[free_epilogue(target1)], lookups=64)]]


LAYOUT = [context(2, 1), context(1, 1), context(2, 0)]


def by_section(cells):
    out = {}
    for c, d, s, x in cells:
        out.setdefault((c, d, s), []).append(x)
    return out


def test_the_sample_of_hand_written_layouts():
    cells = select_cells(LAYOUT, seed=5)
    assert len(set(cells)) == len(cells)                                          # no duplicates
    got = by_section(cells)
    assert {c for c, _, _, _ in cells} == {0, 1, 2}                               # every Context, the middle one included
    for c, digests in enumerate(LAYOUT):
        for d, sections in enumerate(digests):
            for i, s in enumerate(sections):
                g = got[(c, d, s["name"])]
                n = s["cells"]
                assert all(0 <= x < n for x in g)                                 # nothing outside the section
                assert 0 in g and n - 1 in g
                for j in s["jumps"]:                                              # both neighbours of every jump ...
                    if j > 0:
                        assert j - 1 in g
                    else:                                                         # ... the one before the section: its predecessor's last cell
                        prev = sections[i - 1] if i else digests[d - 1][-1]
                        assert prev["cells"] - 1 in got[(c, d - (0 if i else 1), prev["name"])]
                    if j < n:
                        assert j in g
                    else:
                        nxt = sections[i + 1] if i + 1 < len(sections) else digests[d + 1][0]
                        assert 0 in got[(c, d + (0 if i + 1 < len(sections) else 1), nxt["name"])]
                for x in s["free"]:
                    assert x in g                                                 # the free witnesses, on purpose
                if s["zero"] is not None:
                    assert s["zero"] in g
                musts = {0, n - 1} | {x for j in s["jumps"] for x in (j - 1, j) if 0 <= x < n} | set(s["free"]) | ({s["zero"]} - {None})
                assert len(g) == min(n, len(musts) + 8)                           # 8 random cells besides
                lk = got[(c, d, "lookup:" + s["name"])]
                assert all(0 <= x < s["lookups"] for x in lk) and {0, s["lookups"] - 1} <= set(lk)
                assert len(lk) == min(s["lookups"], 2 + 4)
                for fam in ("dense", "spread"):
                    if s["limb_calls"]:
                        ch = got[(c, d, fam + ":" + s["name"])]
                        assert all(0 <= x < s["limb_calls"] for x in ch) and {0, s["limb_calls"] - 1} <= set(ch)
                        assert len(ch) == min(s["limb_calls"], 2 + 4)
                        if s["limb_calls"] > 1:
                            assert {x % 2 for x in ch} == {0, 1}                  # both chip columns (2 columns: call % 2)
                    else:
                        assert (c, d, fam + ":" + s["name"]) not in got
    # the free witnesses differ with the selected round
    assert (0, 0, "epilogue", 76 * 2 + 6) in cells and (1, 0, "epilogue", 76 + 6) in cells and (2, 1, "epilogue", 6) in cells


def test_the_sample_is_seeded():
    a = select_cells(LAYOUT, seed=5)
    assert a == select_cells(LAYOUT, seed=5)
    b = select_cells(LAYOUT, seed=6)
    assert a != b and len(a) == len(b)
    # fewer random cells: the per-section and per-jump cells stay
    small = select_cells(LAYOUT, seed=5, n_random=0, n_random_lookup=0, n_random_chip=0)
    assert set(small) <= set(a) and set(small) <= set(b)
    assert set(small) <= set(select_cells(LAYOUT, seed=5, n_random=2)) <= set(a)


def test_a_one_cell_section_and_a_section_of_nothing_but_musts():
    cells = select_cells([[[sec("prologue", 1, [0, 1]), sec("block0", 3, [1, 2], zero=None, lookups=2, limb_calls=2)]]], seed=1)
    assert sorted(cells) == sorted([(0, 0, "prologue", 0), (0, 0, "block0", 0), (0, 0, "block0", 1), (0, 0, "block0", 2),
                                    (0, 0, "lookup:block0", 0), (0, 0, "lookup:block0", 1),
                                    (0, 0, "dense:block0", 0), (0, 0, "dense:block0", 1), (0, 0, "spread:block0", 0), (0, 0, "spread:block0", 1)])
