"""csrc/ssd_chunks.h by itself: chunk_plan, the points per block of the general chunk and of K1, K2 and K4 that every enqueue takes
(DESIGN.md section 7r), through tests/chunk_plan_main.cpp - a program of its own, built with g++ and run (tests/follow_geometry.py).  Neither a GPU nor the HIP
toolchain is needed: the header includes nothing.

The default tuning over six frame shapes and eight batch sizes.  Every chunk is a whole number of tiles and within its kernel's
bound (the program prints the header's constants: none is copied here), and equals tests/golden/chunk_plan.json - the rules as they
stood inline in enqueue_impl before they had a header, recorded once from that text."""
import json
import os

import pytest

from follow_geometry import build_chunk_plan, chunk_plans

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [64 * 16, 96 * 16, 640 * 480, 848 * 480, 1024 * 768, 1920 * 1080]
FRAMES = [1, 2, 8, 16, 64, 65, 256, 1024]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = build_chunk_plan(tmp_path_factory.mktemp("chunk_plan"))
    return chunk_plans(exe, [(n, f) for n in SHAPES for f in FRAMES])


def test_every_case_has_a_plan(plans):
    _, _, got = plans
    assert sorted(got) == sorted((n, f) for n in SHAPES for f in FRAMES)


def test_chunks_are_whole_tiles_within_their_bounds(plans):
    tile, bounds, got = plans
    assert tile == 1024
    for case, plan in got.items():
        for name, value in plan.items():
            assert value > 0 and value % 1024 == 0, (case, name, value)
            assert value <= bounds[name], (case, name, value, bounds[name])


def test_chunks_equal_the_recorded_plans(plans):
    _, _, got = plans
    with open(os.path.join(HERE, "golden", "chunk_plan.json"), encoding="utf-8") as f:
        golden = json.load(f)
    assert golden["columns"] == ["nPoints", "nframes", "chunk", "hist", "raster", "inquad"]
    want = {(row[0], row[1]): dict(zip(golden["columns"][2:], row[2:])) for row in golden["plans"]}
    assert sorted(want) == sorted(got)
    for case in want:
        assert got[case] == want[case], (case, got[case], want[case])
