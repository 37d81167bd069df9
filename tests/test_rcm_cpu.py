"""Reverse Cuthill-McKee on the CPU (tests/rcm_restatement.py): the queue form and the level-synchronous form agree on every case, the
result is a permutation whose components and breadth-first levels are contiguous, the bandwidths of the shuffled grids come back to
at most their natural numbering's; the ABI surface.  No GPU."""
import os
import re

import numpy as np
import pytest
from rcm_cases import GRIDS, NAMES, rcm_case, restated, shuffle_of
from rcm_restatement import adjacency, bandwidth, bfs_levels, components_of, rcm_queue

from sparse_matrix_math_amd import _lib
from sparse_matrix_math_amd import generators as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smm_hip_csr_rcm", "smm_hip_csr_rcm_dev", "smm_hip_csr_bandwidth")
PROTOTYPE = {"poisson2d_32_shuffled": (1002, 32, 1559, 65, 63), "convdiff3d_12_shuffled": (1685, 114, 2855, 229, 34),
             "poisson3d_20_shuffled": (7909, 310, 13149, 621, 58)}  # bandwidth shuffled / after, offsets shuffled / after, levels


@pytest.mark.parametrize("reverse", [True, False], ids=["rcm", "cm"])
@pytest.mark.parametrize("name", NAMES)
def test_the_two_forms_agree(name, reverse):
    csr = rcm_case(name)
    perm_q, info_q = rcm_queue(csr, reverse)
    perm_l, info_l = restated(name, reverse)
    np.testing.assert_array_equal(perm_q, perm_l)
    assert info_q == info_l
    np.testing.assert_array_equal(restated(name, True)[0], restated(name, False)[0][::-1])


@pytest.mark.parametrize("name", NAMES)
def test_permutation_components_and_levels_are_contiguous(name):
    csr = rcm_case(name)
    n = len(csr[0]) - 1
    order, info = restated(name, False)  # Cuthill-McKee: the order the components were numbered in
    np.testing.assert_array_equal(np.sort(order), np.arange(n))
    label = components_of(csr)[order] if n else np.zeros(0, dtype=np.int64)
    bounds = np.flatnonzero(np.diff(label)) + 1
    assert len(bounds) + (1 if n else 0) == len(np.unique(label)) == info["components"]  # a label never comes back: contiguous
    astart, apos = adjacency(csr)
    deepest = 0
    for first, last in zip(np.concatenate([[0], bounds]) if n else [], np.concatenate([bounds, [n]]) if n else []):
        levels = bfs_levels(astart, apos, int(order[first]), np.zeros(n, dtype=bool))
        depth_of = {v: d for d, level in enumerate(levels) for v in level}
        depths = [depth_of[int(v)] for v in order[first:last]]
        assert depths == sorted(depths) and depths[-1] == len(levels) - 1
        deepest = max(deepest, len(levels))
    assert deepest == info["levels"]


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_shuffled_grids_come_back_to_their_natural_bandwidth(name):
    csr = rcm_case(name)
    perm, info = restated(name)
    shuffled, after, offsets_shuffled, offsets_after, levels = PROTOTYPE[name]
    got = (info["bandwidth_before"], info["bandwidth_after"], bandwidth(csr)[1], bandwidth(csr, perm)[1], info["levels"])
    print(name, "bandwidth / offsets / levels", got, "natural", GRIDS[name])
    assert info["bandwidth_after"] <= GRIDS[name]
    assert got == (shuffled, after, offsets_shuffled, offsets_after, levels)  # the issue's table


def test_the_one_sided_path_gets_bandwidth_one():
    perm, info = restated("bidiagonal_300")
    assert info == {"components": 1, "levels": 300, "bandwidth_before": 1, "bandwidth_after": 1}
    assert perm[0] in (0, 299) and abs(int(perm[-1]) - int(perm[0])) == 299  # the root moved to an end


def test_isolated_vertices_come_first_in_index_order():
    order, info = restated("dense70_in_200", False)
    np.testing.assert_array_equal(order[:130], np.concatenate([np.arange(40), np.arange(110, 200)]))
    assert info["components"] == 131 and info["levels"] == 2
    order, info = restated("diagonal_100000", False)
    np.testing.assert_array_equal(order, np.arange(100000))
    assert info == {"components": 100000, "levels": 1, "bandwidth_before": 0, "bandwidth_after": 0}
    assert restated("empty")[1] == {"components": 0, "levels": 0, "bandwidth_before": 0, "bandwidth_after": 0}
    assert restated("one")[1]["levels"] == 1


def test_shuffled_40_cubed_laplacian_exceeds_the_codes_dictionary_until_reordered():
    csr = gen.poisson3d(40)
    shuffle = shuffle_of(64000)
    assert bandwidth(csr) == (1600, 7)
    assert bandwidth(csr, shuffle) == (63780, 106203)  # more offsets than the CODES encoding's 65536


def test_abi_declares_and_binds_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "smm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", text), name
        assert name in _lib._PLAIN, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
