"""CPU tests of the mesh export chain's argument layer (mast3r_slam/tsdf/mesh_chain.py, DESIGN.md "Mesh export chain"):
the option table, and what each of the five functions that take `**chain` hands on, through fakes that record the call.
The bow-tie and decimation rows are in test_mesh_bowties_cpu.py and test_mesh_decimate_cpu.py; test_mesh_chain_gpu.py
runs the five stages."""
import inspect
import types

import numpy as np
import pytest

# the 13 options in the order the stages run, with their defaults
TABLE = (("min_component_faces", 0), ("keep_largest", None),
         ("fill_holes", 0), ("fill_bowties", False),
         ("smooth_iterations", 0), ("smooth_lambda", 0.5), ("smooth_mu", -0.53), ("smooth_boundary", "fixed"),
         ("simplify_cell", 0.0), ("simplify_position", "quadric"),
         ("decimate_faces", None), ("decimate_ratio", None), ("decimate_error", None))
STAGES = (("components", 2), ("fill", 2), ("smooth", 4), ("simplify", 2), ("decimate", 3))
OWN = ("min_weight", "level", "colors", "default_color")
VS = 0.03

SMOOTH = dict(smooth_lambda=0.5, smooth_mu=-0.53, smooth_boundary="fixed")
# (given, handed on): a stage that is on goes with all its options, one that is off does not go at all
ROWS = (
    ({}, {}),
    (dict(min_component_faces=50), dict(min_component_faces=50, keep_largest=None)),
    (dict(keep_largest=1), dict(min_component_faces=0, keep_largest=1)),
    (dict(keep_largest=0), dict(min_component_faces=0, keep_largest=0)),
    (dict(min_component_faces=0), {}),
    (dict(min_component_faces=0, keep_largest=None), {}),
    (dict(fill_holes=8), dict(fill_holes=8)),
    (dict(fill_holes=8, fill_bowties=True), dict(fill_holes=8, fill_bowties=True)),
    (dict(fill_holes=8, fill_bowties=np.True_), dict(fill_holes=8, fill_bowties=True)),
    (dict(fill_holes=None, fill_bowties=True), {}),
    (dict(smooth_iterations=3), dict(smooth_iterations=3, **SMOOTH)),
    (dict(smooth_iterations=3, smooth_lambda=0.4), dict(SMOOTH, smooth_iterations=3, smooth_lambda=0.4)),
    (dict(smooth_iterations=3, smooth_mu=0.0), dict(SMOOTH, smooth_iterations=3, smooth_mu=0.0)),
    (dict(smooth_iterations=3, smooth_boundary="curve"), dict(SMOOTH, smooth_iterations=3, smooth_boundary="curve")),
    (dict(smooth_iterations=0, smooth_lambda=0.4, smooth_mu=0.0, smooth_boundary="free"), {}),
    (dict(smooth_iterations=None), {}),
    (dict(simplify_cell=0.06), dict(simplify_cell=0.06, simplify_position="quadric")),
    (dict(simplify_cell=0.06, simplify_position="mean"), dict(simplify_cell=0.06, simplify_position="mean")),
    (dict(simplify_cell=0.0, simplify_position="mean"), {}),
    (dict(simplify_cell=None), {}),
    (dict(decimate_faces=500), dict(decimate_faces=500)),
    (dict(decimate_ratio=0.2), dict(decimate_ratio=0.2)),
    (dict(decimate_error=0.01), dict(decimate_error=0.01)),
    (dict(decimate_faces=0, decimate_ratio=None, decimate_error=-1.0), {}),
    (dict(keep_largest=1, fill_holes=64, fill_bowties=True, smooth_iterations=2, simplify_cell=0.06, decimate_ratio=0.5),
     dict(min_component_faces=0, keep_largest=1, fill_holes=64, fill_bowties=True, smooth_iterations=2, **SMOOTH,
          simplify_cell=0.06, simplify_position="quadric", decimate_ratio=0.5)),
)
# (tsdf_global, given, handed on) for SlamSystem.extract_mesh: absent or None takes the config's value
SYSTEM_ROWS = (
    (dict(mesh_min_component_faces=50), {}, dict(min_component_faces=50, keep_largest=None)),
    (dict(mesh_min_component_faces=50), dict(min_component_faces=None), dict(min_component_faces=50, keep_largest=None)),
    (dict(mesh_min_component_faces=50), dict(min_component_faces=0), {}),
    (dict(mesh_min_component_faces=50), dict(keep_largest=2), dict(min_component_faces=50, keep_largest=2)),
    (dict(mesh_simplify_voxels=2.0), {}, dict(simplify_cell=2.0 * VS, simplify_position="quadric")),
    (dict(mesh_simplify_voxels=2.0), dict(simplify_position="mean"), dict(simplify_cell=2.0 * VS, simplify_position="mean")),
    (dict(mesh_simplify_voxels=2.0), dict(simplify_cell=0.0), {}),
    (dict(mesh_simplify_voxels=2.0), dict(simplify_cell=0.1), dict(simplify_cell=0.1, simplify_position="quadric")),
    (dict(mesh_smooth_iterations=5), {}, dict(smooth_iterations=5, **SMOOTH)),
    (dict(mesh_smooth_iterations=5), dict(smooth_mu=0.0), dict(SMOOTH, smooth_iterations=5, smooth_mu=0.0)),
    (dict(mesh_smooth_iterations=5), dict(smooth_iterations=0), {}),
    (dict(mesh_fill_holes=8), {}, dict(fill_holes=8)),
    (dict(mesh_fill_holes=8), dict(fill_holes=0), {}),
    (dict(mesh_fill_holes=8, mesh_fill_bowties=True), {}, dict(fill_holes=8, fill_bowties=True)),
    (dict(mesh_fill_holes=8, mesh_fill_bowties=True), dict(fill_bowties=False), dict(fill_holes=8)),
    (dict(mesh_decimate_faces=1000), {}, dict(decimate_faces=1000)),
    (dict(mesh_decimate_faces=1000), dict(decimate_faces=0), {}),
    (dict(mesh_decimate_error=0.5), {}, dict(decimate_error=0.5 * VS)),
    (dict(mesh_decimate_error=0.5), dict(decimate_error=0.0), {}),
)


def _chain(kw):
    return {k: v for k, v in kw.items() if k not in OWN}


@pytest.fixture
def levels(tmp_path, monkeypatch):
    """name -> f(**given) -> the chain options that the function hands to the level below it."""
    from mast3r_slam import evaluate, tsdf
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import global_volume

    calls = []
    record = lambda **kw: calls.append(kw) or "mesh"
    # a sharded volume with colours hands on to the union of its shards
    sharded = types.SimpleNamespace(min_weight=0.5, color=True, num_shards=2,
                                    _union=lambda: types.SimpleNamespace(extract_mesh=record))
    sharded.extract_mesh = lambda **kw: tsdf.TSDFVolume.extract_mesh(sharded, **kw)
    volume = types.SimpleNamespace(voxel_size=VS, extract_mesh=record)
    manager = types.SimpleNamespace(volume=volume, cfg={})
    manager.extract_mesh = lambda **kw: tsdf.TSDFGlobalManager.extract_mesh(manager, **kw)
    system = types.SimpleNamespace(tsdf_manager=manager, drain=lambda: None)
    monkeypatch.setattr(global_volume, "_loaded", lambda *a: types.SimpleNamespace(extract_mesh=record))

    class Source:
        def extract_mesh(self, **kw):
            calls.append(kw)
            raise LookupError

    def save(**given):
        with pytest.raises(LookupError):
            evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", Source(), **given)

    fns = {"TSDFVolume.extract_mesh": lambda **given: sharded.extract_mesh(colors=True, **given),
           "mesh_from_voxels": lambda **given: tsdf.mesh_from_voxels(None, None, None, VS, 0.5, **given),
           "TSDFGlobalManager.extract_mesh": manager.extract_mesh,
           "save_tsdf_mesh": save,
           "SlamSystem.extract_mesh": lambda **given: SlamSystem.extract_mesh(system, **given)}

    def handed_on(fn):
        def f(**given):
            fn(**given)
            assert len(calls) == 1
            return _chain(calls.pop())
        return f

    out = {name: handed_on(fn) for name, fn in fns.items()}
    out["cfg"] = manager
    return out


def _functions():
    from mast3r_slam import evaluate, tsdf
    from mast3r_slam.slam_system import SlamSystem

    method = ("self", "min_weight", "level", "colors")
    return {tsdf.TSDFVolume.extract_mesh: method + ("default_color",),
            tsdf.mesh_from_voxels: ("keys", "tsdf", "weight", "voxel_size", "min_weight", "level", "device", "colors",
                                    "default_color"),
            tsdf.TSDFGlobalManager.extract_mesh: method,
            evaluate.save_tsdf_mesh: ("savedir", "filename", "source", "min_weight", "level", "colors"),
            SlamSystem.extract_mesh: method}


def test_the_option_table():
    from mast3r_slam.config import config
    from mast3r_slam.tsdf import mesh_chain

    assert tuple(mesh_chain.DEFAULTS.items()) == TABLE and len(TABLE) == 13
    assert tuple((stage, len(options)) for stage, options in mesh_chain.OPTIONS.items()) == STAGES
    assert [name for options in mesh_chain.OPTIONS.values() for name in options] == [name for name, _ in TABLE]
    for name, default in TABLE:                                      # 0, 0.0 and False are equal to each other
        assert type(mesh_chain.DEFAULTS[name]) is type(default), name
    keys = {name: key for name, (key, _, _) in mesh_chain.CONFIG.items()}
    assert keys == dict(min_component_faces="mesh_min_component_faces", simplify_cell="mesh_simplify_voxels",
                        smooth_iterations="mesh_smooth_iterations", fill_holes="mesh_fill_holes",
                        fill_bowties="mesh_fill_bowties", decimate_faces="mesh_decimate_faces",
                        decimate_error="mesh_decimate_error")
    assert {name for name, (_, _, in_voxels) in mesh_chain.CONFIG.items() if in_voxels} == {"simplify_cell", "decimate_error"}
    for name, (key, kind, _) in mesh_chain.CONFIG.items():          # the shipped config leaves every stage off
        assert type(config["tsdf_global"][key]) is kind and not config["tsdf_global"][key], key


def test_named_parameters_are_each_function_s_own():
    for fn, own in _functions().items():
        p = inspect.signature(fn).parameters
        assert tuple(k for k, v in p.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD) == own, fn
        assert [v.kind for k, v in p.items() if k not in own] == [inspect.Parameter.VAR_KEYWORD], fn
        assert not set(p) & {name for name, _ in TABLE}, fn


def test_rows_cover_every_option():
    assert {name for given, _ in ROWS for name in given} == {name for name, _ in TABLE}
    for name, default in TABLE:                                      # ... each one handed on at a value of its own
        assert any(name in passed and passed[name] is not default and passed[name] != default for _, passed in ROWS), name


@pytest.mark.parametrize("fn", ["TSDFVolume.extract_mesh", "mesh_from_voxels", "TSDFGlobalManager.extract_mesh",
                                "save_tsdf_mesh", "SlamSystem.extract_mesh"])
def test_what_is_on_is_handed_on(levels, fn):
    """Every option is accepted by keyword; left out, or off, nothing of its stage goes on; on, all of its stage does,
    the others at the table's defaults."""
    for given, passed in ROWS:
        if fn == "mesh_from_voxels":                                 # hands on as given: the volume behind it decides
            passed = given
        got = levels[fn](**given)
        assert got == passed and all(type(got[k]) is type(passed[k]) for k in got), (given, got)
        if fn != "mesh_from_voxels":
            assert levels[fn](**got) == got                          # the level below sees the same again


def test_system_defaults_come_from_the_config(levels):
    for cfg, given, passed in SYSTEM_ROWS:
        levels["cfg"].cfg = cfg
        assert levels["SlamSystem.extract_mesh"](**given) == passed, (cfg, given)


@pytest.mark.parametrize("fn,what", [("TSDFVolume.extract_mesh", "TSDFVolume.extract_mesh"),
                                     ("TSDFGlobalManager.extract_mesh", "TSDFGlobalManager.extract_mesh"),
                                     ("save_tsdf_mesh", "save_tsdf_mesh")])
def test_messages(fn, what):
    from mast3r_slam.tsdf.mesh_chain import chain_options

    for bad in ("fill_bow_ties", "decimate_face", "smooth", "min_weight"):
        with pytest.raises(TypeError, match=rf"{what}\(\) got an unexpected keyword argument '{bad}'"):
            chain_options({bad: 1}, what)
    for bad in (1, 0, None, "on", 1.0):
        for fill in (8, 0):                                          # fill on or off
            with pytest.raises(ValueError, match=f"{what}: fill_bowties must be a bool, got {bad!r}"):
                chain_options(dict(fill_holes=fill, fill_bowties=bad), what)


def test_messages_through_the_functions(levels):
    for fn, what in (("TSDFVolume.extract_mesh", "TSDFVolume.extract_mesh"),
                     ("TSDFGlobalManager.extract_mesh", "TSDFGlobalManager.extract_mesh"),
                     ("save_tsdf_mesh", "save_tsdf_mesh"), ("SlamSystem.extract_mesh", "TSDFGlobalManager.extract_mesh")):
        with pytest.raises(TypeError, match=rf"{what}\(\) got an unexpected keyword argument 'fill_bow_ties'"):
            levels[fn](fill_holes=8, fill_bow_ties=True)
        with pytest.raises(TypeError, match="unexpected keyword argument 'decimate_face'"):
            levels[fn](decimate_face=500)
        with pytest.raises(ValueError, match=f"{what}: fill_bowties must be a bool"):
            levels[fn](fill_holes=8, fill_bowties="on")
        with pytest.raises(ValueError, match=f"{what}: fill_bowties must be a bool"):
            levels[fn](fill_bowties=1)
