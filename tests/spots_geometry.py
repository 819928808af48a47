"""How the trap-list kernels cut their work, restated in plain Python from
csrc/spots.hip (plan_fields and the fold of spot_update_kernel), and the table
of shapes whose tests run those cuts beyond their first pass. The device tests
first compare Spots.info() with geometry(), so a change of the split heuristic
shows here, on the CPU, before it turns a case back into a single-chunk one.
Test infrastructure only."""
from collections import namedtuple

TILE = 32            # MFMA tile side: traps are padded to it, columns are cut in chunks of it
WAVES = 4            # row tiles per workgroup of the fields product
TARGET_WAVES = 4096  # columns are split until a hologram has this many waves
UPDATE_THREADS = 1024
FOLD_LOADS = 8       # partials one fold group adds per round
GRID_CAP = 8192 * 256  # elements one pass of the grid-stride kernels covers

Geometry = namedtuple("Geometry", "padded_traps col_splits cols_per_partial partials fold_groups fold_rounds "
                                  "last_split_cols table_elements")


def _ceil_div(a, b):
    return -(-a // b)


def geometry(h, w, m):
    mp = _ceil_div(m, TILE) * TILE
    row_tiles, chunks = _ceil_div(h, TILE), _ceil_div(w, TILE)
    trap_tiles = mp // TILE
    splits = max(1, min(_ceil_div(TARGET_WAVES, row_tiles * trap_tiles), chunks))
    chunks_per = _ceil_div(chunks, splits)
    col_splits = _ceil_div(chunks, chunks_per)
    cols = chunks_per * TILE
    partials = _ceil_div(row_tiles, WAVES) * col_splits
    groups = UPDATE_THREADS // mp
    return Geometry(mp, col_splits, cols, partials, groups, _ceil_div(partials, FOLD_LOADS * groups),
                    w - (col_splits - 1) * cols, 2 * (h + w) * mp)


# (H, W, M) -> (col splits, cols per partial, partials, fold rounds) as the case was chosen, and what it is there for
CASES = {
    (1080, 1920, 5): ((60, 32, 540, 3), "the panel with few traps: the fold with 32 groups wraps"),
    (1080, 1920, 100): ((30, 64, 270, 5), "two chunks per split, 8 fold groups"),
    (1080, 1920, 1024): ((4, 480, 36, 5), "the longest chain: 15 chunks per split"),
    (2048, 71, 1024): ((2, 64, 32, 4), "last split 7 columns wide, odd width, two passes of the tables kernel"),
    (4096, 45, 1000): ((1, 64, 32, 4), "maximum height, a split wider than the image, M below its padding"),
    (34, 4096, 1024): ((64, 64, 64, 8), "maximum width, a 2-row second row tile, waves 2 and 3 all zeros"),
    (512, 530, 1024): ((6, 96, 24, 3), "three chunks per split, last split 50 columns"),
    (257, 97, 1023): ((4, 32, 12, 2), "last split 1 column, a row group holding a single row"),
    (2, 4096, 33): ((128, 32, 128, 1), "partials == 8 * groups exactly, height 2"),
    (2, 2, 1): ((1, 32, 1, 1), "minimum sides"),
    (3, 33, 31): ((2, 32, 2, 1), "one below the padding boundary, last split 1 column"),
    (3, 33, 32): ((2, 32, 2, 1), "at the padding boundary"),
    (3, 33, 33): ((2, 32, 2, 1), "one above the padding boundary"),
}


def case_id(case):
    return "%dx%d-%d" % case
