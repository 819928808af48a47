"""The shapes of tests/test_gpu_spots_geometry.py still reach what they are
there for: tests/spots_geometry.py restates how csrc/spots.hip cuts the fields
product and folds its partial sums, and every case of its table is held to the
property it was chosen for (more than one chunk per column split, a ragged
last split after a full one, a fold that wraps, a second grid-stride pass). A
change of the split heuristic that turns a case back into a single-chunk one
fails here and names the case; the device tests compare the same prediction
with Spots.info()."""
import pytest

import spots_geometry as sg

# what each case must keep: (what it is, predicate on (h, w, m, geometry))
PROPERTIES = {
    (1080, 1920, 5): [
        ("padded to one trap tile, 32 fold groups", lambda h, w, m, g: g.padded_traps == 32 and g.fold_groups == 32),
        ("the fold wraps: 3 rounds or more", lambda h, w, m, g: g.fold_rounds >= 3),
        ("a batch of two passes the phase kernel's grid twice", lambda h, w, m, g: 2 * h * w > sg.GRID_CAP),
    ],
    (1080, 1920, 100): [
        ("two chunks per split", lambda h, w, m, g: g.cols_per_partial == 2 * sg.TILE),
        ("8 fold groups, 3 rounds or more", lambda h, w, m, g: g.fold_groups == 8 and g.fold_rounds >= 3),
    ],
    (1080, 1920, 1024): [
        ("480 columns or more per partial", lambda h, w, m, g: g.cols_per_partial >= 480),
        ("3 fold rounds or more", lambda h, w, m, g: g.fold_rounds >= 3),
    ],
    (2048, 71, 1024): [
        ("a split wider than one chunk", lambda h, w, m, g: g.cols_per_partial > sg.TILE),
        ("a narrower last split after a full one",
         lambda h, w, m, g: g.col_splits >= 2 and 0 < g.last_split_cols < g.cols_per_partial),
        ("odd width", lambda h, w, m, g: w % 2 == 1),
        ("the tables kernel passes its grid twice", lambda h, w, m, g: g.table_elements > sg.GRID_CAP),
        ("3 fold rounds or more", lambda h, w, m, g: g.fold_rounds >= 3),
    ],
    (4096, 45, 1000): [
        ("maximum height", lambda h, w, m, g: h == 4096),
        ("one split, wider than the image", lambda h, w, m, g: g.col_splits == 1 and g.cols_per_partial > w),
        ("M below its padding", lambda h, w, m, g: m < g.padded_traps),
    ],
    (34, 4096, 1024): [
        ("maximum width", lambda h, w, m, g: w == 4096),
        ("two row tiles, the second of 2 rows: waves 2 and 3 see zeros",
         lambda h, w, m, g: h == sg.TILE + 2 and g.partials == g.col_splits),
        ("3 fold rounds or more", lambda h, w, m, g: g.fold_rounds >= 3),
    ],
    (512, 530, 1024): [
        ("three chunks per split", lambda h, w, m, g: g.cols_per_partial == 3 * sg.TILE),
        ("last split 50 columns after a full one", lambda h, w, m, g: g.col_splits >= 2 and g.last_split_cols == 50),
        ("3 fold rounds or more", lambda h, w, m, g: g.fold_rounds >= 3),
    ],
    (257, 97, 1023): [
        ("last split 1 column after a full one", lambda h, w, m, g: g.col_splits >= 2 and g.last_split_cols == 1),
        ("the last row group holds a single row", lambda h, w, m, g: h % (sg.WAVES * sg.TILE) == 1),
        ("the fold wraps", lambda h, w, m, g: g.fold_rounds >= 2),
        ("one trap below the padding", lambda h, w, m, g: m == g.padded_traps - 1),
    ],
    (2, 4096, 33): [
        ("partials == 8 * groups exactly", lambda h, w, m, g: g.partials == sg.FOLD_LOADS * g.fold_groups),
        ("height 2", lambda h, w, m, g: h == 2),
    ],
    (2, 2, 1): [("minimum sides, one trap", lambda h, w, m, g: (h, w, m) == (2, 2, 1) and g.partials == 1)],
    (3, 33, 31): [
        ("one below the padding boundary", lambda h, w, m, g: m == g.padded_traps - 1),
        ("last split 1 column", lambda h, w, m, g: g.col_splits == 2 and g.last_split_cols == 1),
    ],
    (3, 33, 32): [
        ("at the padding boundary", lambda h, w, m, g: m == g.padded_traps),
        ("last split 1 column", lambda h, w, m, g: g.col_splits == 2 and g.last_split_cols == 1),
    ],
    (3, 33, 33): [
        ("one above the padding boundary", lambda h, w, m, g: m == g.padded_traps - sg.TILE + 1),
        ("last split 1 column", lambda h, w, m, g: g.col_splits == 2 and g.last_split_cols == 1),
    ],
}


def test_every_case_has_its_properties():
    assert set(PROPERTIES) == set(sg.CASES)


@pytest.mark.parametrize("case", list(sg.CASES), ids=sg.case_id)
def test_case_still_covers_its_target(case):
    g = sg.geometry(*case)
    print(f"[spots geometry] {sg.case_id(case)}: {g}")
    for what, holds in PROPERTIES[case]:
        assert holds(*case, g), f"{sg.case_id(case)} no longer covers its target ({what}): {g}"
    # the cut the case was chosen at (the table of the issue that added it)
    assert (g.col_splits, g.cols_per_partial, g.partials, g.fold_rounds) == sg.CASES[case][0], (
        f"{sg.case_id(case)} ({sg.CASES[case][1]}) is cut differently now: {g}")


def test_the_table_as_a_whole():
    gs = [sg.geometry(*case) for case in sg.CASES]
    assert sum(g.cols_per_partial >= 480 for g in gs) >= 1
    assert sum(g.col_splits >= 2 and g.last_split_cols < g.cols_per_partial for g in gs) >= 1
    assert sum(g.fold_rounds >= 3 for g in gs) >= 3
    assert sum(g.partials == sg.FOLD_LOADS * g.fold_groups for g in gs) >= 1


def test_shapes_the_suite_had_before_are_single_chunk():
    """What the new table adds: every shape of test_gpu_spots.py runs the K loop
    once and never wraps the fold."""
    for case in ((45, 70, 5), (64, 64, 1), (96, 160, 33), (130, 264, 70), (64, 64, 1024)):
        g = sg.geometry(*case)
        assert g.cols_per_partial == sg.TILE and g.fold_rounds == 1 and g.partials <= 18
