"""Regenerates tests/golden/slab_plans.json: every plan cuda_mesh_voxelization_amd/slab.py makes for the splits of PLAN_SIDES x PLAN_WORLDS that
slab_range accepts -- this project's own output, integers only.  tests/test_slab_cpu.py compares slab.py with it (record() is what both run)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PLAN_SIDES, PLAN_WORLDS = (96, 128, 160, 256, 1152), (1, 2, 3, 4, 8)


def record(S):
    """S: the slab module.  {"n/world": {"halo": [[[src, dst, side (0 minus, 1 plus), g0, g1], ...] per step n/2 ... 1], "ranks": [per rank {...}]}}"""
    ints = lambda v: json.loads(json.dumps(v))                    # tuples -> lists, as the file holds them
    out = {}
    for n in PLAN_SIDES:
        for world in PLAN_WORLDS:
            try:
                S.slab_range(n, 0, world)
            except ValueError:
                continue
            ks = [k for k, _, _ in S.ghost_regions(n, 0, world)]
            halo = [[[s, t, int(side == "plus"), g0, g1] for s, t, side, g0, g1 in S.halo_plan(n, world, k)] for k in ks]
            ranks = []
            for r in range(world):
                ranks.append({"ghost": S.ghost_regions(n, r, world), "hybrid": S.hybrid_plan(n, r, world),
                              "window": [S.hybrid_window(n, r, world, False), S.hybrid_window(n, r, world, True)],
                              "transpose": S.transpose_plan(n, r, world), "cyclic": S.cyclic_passes(n, world)})
            out["%d/%d" % (n, world)] = ints({"halo": halo, "ranks": ranks})
    return out


if __name__ == "__main__":
    from cuda_mesh_voxelization_amd import slab
    with open(os.path.join(ROOT, "tests", "golden", "slab_plans.json"), "w") as f:
        json.dump(record(slab), f, separators=(",", ":"))
        f.write("\n")
