"""Interior fill without a GPU: the numpy reference of tests/fill_ref.py against scipy.ndimage.binary_fill_holes and against hand-written
expectations; the host flood of `vpcli --fill` (-t 0 / -t 3, vplib/src/fill.cpp) against the numpy reference on mesh grids; the -g > 1
refusal; idempotence and O contains W."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fill_ref import bool_to_words, fill_numpy, hand_cases, maze, random_grid, words_to_bool  # noqa: E402


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_reference_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for i in range(50):
        n = 32 if i % 5 else 64
        density = float(rng.uniform(0.05, 0.85))
        words = random_grid(n, density, 77 + i)
        exp = ndimage.binary_fill_holes(words_to_bool(words, n))
        got = words_to_bool(fill_numpy(words, n), n)
        assert np.array_equal(got, exp), (i, n, density)


@pytest.mark.parametrize("n", [32, 64, 96])
def test_reference_gets_the_hand_cases_right(n):
    names = set()
    for name, vox, exp in hand_cases(n):
        names.add(name)
        assert np.array_equal(words_to_bool(fill_numpy(bool_to_words(vox), n), n), exp), (n, name)
    assert {"empty", "full", "shell", "shell with a hole", "nested shells", "diagonal gaps (edge)", "diagonal gaps (corner)"} <= names


def test_reference_fills_the_maze_cavities_only():
    n = 64
    words, length = maze(n, seed=3)
    out, steps = fill_numpy(words, n, return_steps=True)
    vox, got = words_to_bool(words, n), words_to_bool(out, n)
    added = got & ~vox
    assert added.sum() >= 1 and (added.sum() == np.count_nonzero(added[::2, ::2, ::2]))   # only the isolated even-coordinate cavities
    assert steps >= length                                   # one dilation step per corridor voxel


def test_fill_is_idempotent_and_contains_the_input():
    for n, density, seed in ((32, 0.3, 1), (64, 0.6, 2), (64, 0.7, 3), (96, 0.69, 4)):
        words = random_grid(n, density, seed)
        once = fill_numpy(words, n)
        assert np.array_equal(once & words, words)
        assert np.array_equal(fill_numpy(once, n), once)


def _vpcli(cli, tmp_path, args, tag):
    prefix = str(tmp_path / tag)
    p = subprocess.run([cli] + args + ["-d", prefix], capture_output=True, text=True, timeout=1800, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return np.fromfile(prefix + ".grid.u32", np.uint32), p.stdout


@pytest.mark.parametrize("name", ["sphere.obj", "torus.obj", "d20.obj", "bimba.obj"])
def test_host_flood_equals_the_reference_on_conservative_grids(cli, tmp_path, name):
    for n in (32, 64):
        surf, _ = _vpcli(cli, tmp_path, [M.asset(name), "-n", str(n), "-t", "0", "--conservative"], "surf")
        exp = fill_numpy(surf, n)
        assert not np.array_equal(exp, surf), (name, n)       # closed meshes: the fill adds the body
        for t in ("0", "3"):
            got, out = _vpcli(cli, tmp_path, [M.asset(name), "-n", str(n), "-t", t, "--conservative", "--fill"], "fill" + t)
            assert np.array_equal(got, exp), (name, n, t, int(np.count_nonzero(got != exp)))
            assert "Fill]: " in out


def test_host_flood_equals_the_reference_on_a_solid_grid(cli, tmp_path):
    n = 64
    solid, _ = _vpcli(cli, tmp_path, [M.asset("bunny.obj"), "-n", str(n), "-t", "0"], "solid")
    exp = fill_numpy(solid, n)
    for t in ("0", "3"):
        got, _ = _vpcli(cli, tmp_path, [M.asset("bunny.obj"), "-n", str(n), "-t", t, "--fill"], "fill" + t)
        assert np.array_equal(got, exp), t


def test_fill_refuses_several_gpus(cli, tmp_path):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "2", "--fill", "-g", "2"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert p.returncode != 0
    assert "--fill runs on one device" in p.stdout + p.stderr


def test_flag_ring_index_arithmetic(tmp_path):
    """tests/cpp/round_ring_check.cpp: where a round's flag lives and which flag it reads (csrc/round_ring.h), as a plain host program"""
    exe = str(tmp_path / "round_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", build.CSRC,
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "round_ring_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-2000:] + p.stderr[-2000:]
