"""GPU test (-m gpu) of the mesh export chain (mast3r_slam/tsdf/mesh_chain.py, DESIGN.md "Mesh export chain"): all five
stages in one call against their composition by hand, bit for bit, through the volume, mesh_from_voxels and the
manager, on a fixture at which every stage changes the mesh."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holes_numpy as H  # noqa: E402
import mc_numpy as M  # noqa: E402
from mesh_support import _same  # noqa: E402

pytestmark = pytest.mark.gpu

VS, TRUNC = 0.03, 0.09
SMALL_C, SMALL_R = np.array([1.1, -0.2, 0.1]), 0.12                  # beside the holed sphere (centre x 0.3, radius 0.31)
CHAIN = dict(keep_largest=1, fill_holes=64, fill_bowties=True, smooth_iterations=2, simplify_cell=2 * VS,
             decimate_ratio=0.5)


def _changed(before, after):
    """A stage did something: another vertex or face count, or other bytes."""
    if before[0].shape != after[0].shape or before[2].shape != after[2].shape:
        return True
    return not all(torch.equal(a, b) for a, b in zip(before, after))


def test_all_five_stages_in_their_order(device):
    from mast3r_slam.tsdf import (TSDFGlobalManager, TSDFVolume, decimate_mesh, fill_holes, filter_mesh,
                                  mesh_from_voxels, simplify_mesh, smooth_mesh)

    big = H.sphere_voxels(0, 200)
    small = M.sample_sdf(M.sphere_sdf(SMALL_C, SMALL_R), SMALL_C - SMALL_R, SMALL_C + SMALL_R, VS, TRUNC)
    gap = np.maximum(small[0].min(0) - big[0].max(0), big[0].min(0) - small[0].max(0)).max()
    assert gap >= 4, gap                                             # empty voxels between the two: bounding boxes of keys
    keys, t, w = (np.concatenate([a, b]) for a, b in zip(big, small))
    vol = TSDFVolume(VS, TRUNC, 100.0, 0.5, capacity=1 << 15, device=device)
    vol.load_voxels(keys, t, w)

    plain = vol.extract_mesh()
    stages = [plain, filter_mesh(plain, keep_largest=1)]
    stages.append(fill_holes(stages[-1], 64, bowties=True))
    stages.append(smooth_mesh(stages[-1], 2))
    stages.append(simplify_mesh(stages[-1], 2 * VS))
    stages.append(decimate_mesh(stages[-1], ratio=0.5))
    for name, before, after in zip(("filter", "fill", "smooth", "simplify", "decimate"), stages, stages[1:]):
        print(f"{name}: {before[0].shape[0]} / {before[2].shape[0]} -> {after[0].shape[0]} / {after[2].shape[0]}")
        assert _changed(before, after), name                         # a stage that is silently off cannot pass
    want = stages[-1]

    got = vol.extract_mesh(**CHAIN)
    assert len(got) == 3
    _same(got, want)
    _same(mesh_from_voxels(keys, t, w, VS, 0.5, device=device, **CHAIN), want)
    manager = types.SimpleNamespace(volume=vol, cfg={})
    _same(TSDFGlobalManager.extract_mesh(manager, **CHAIN), want)
    _same(vol.extract_mesh(), plain)                                 # and the defaults leave the mesh as extracted
