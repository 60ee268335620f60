"""The mesh export chain: the stages that every extract_mesh, mesh_from_voxels and evaluate.save_tsdf_mesh run on the
extracted (and coloured) mesh, their options and their order (DESIGN.md "Mesh export chain").  Those functions take the
options below as keywords (`**chain`) and know nothing else about them.  In the order the stages run:

`min_component_faces` > 0 / `keep_largest`=k: connected components with fewer faces / all but the k largest are dropped
(mesh_ops.filter_mesh, DESIGN.md "Mesh components"; one more host read).  First, so floaters are dropped before anything
could merge them into the surface.
`fill_holes` = n > 0: boundary loops of at most n edges that are holes are closed with a centroid fan
(mesh_holes.fill_holes, DESIGN.md "Mesh holes"; four more host reads), before the smoothing, which then fairs the
patches.  `fill_bowties=True`: holes that meet in a vertex, as two diagonal missing voxels leave them, are told apart and
closed too (fill_holes' bow-tie mode; no further host read); without `fill_holes` it does nothing.
`smooth_iterations` > 0: that many Taubin iterations with `smooth_lambda`, `smooth_mu`, `smooth_boundary`
(mesh_smooth.smooth_mesh, DESIGN.md "Mesh smoothing"; two more host reads), before the simplification, whose plane
quadrics then see the smoothed surface; normals are recomputed.
`simplify_cell` > 0 (world units; a whole number of voxels keeps the cells aligned with them): the mesh is simplified by
clustering its vertices on that grid, placed by `simplify_position` = "quadric" | "mean" (mesh_simplify.simplify_mesh,
DESIGN.md "Mesh simplification"; three more host reads).
`decimate_faces` = n > 0 / `decimate_ratio` in (0, 1] / `decimate_error` > 0 (world units): the mesh is decimated by edge
collapses to n faces / that share of its faces / while the quadric error allows (mesh_decimate.decimate_mesh, DESIGN.md
"Mesh decimation"; two host reads and one more per round).  Last, after the cluster simplification, so both can be
combined.

Every stage is off by default and leaves the mesh as it is; a stage that is off is not handed on to the next level.
SlamSystem.extract_mesh takes an option that is absent or None from tsdf_global (CONFIG below)."""
from ._mesh_args import _bool_arg
from .mesh_decimate import decimate_mesh
from .mesh_holes import fill_holes
from .mesh_ops import filter_mesh
from .mesh_simplify import simplify_mesh
from .mesh_smooth import smooth_mesh

# stage -> its options and their defaults, in the order the stages run
OPTIONS = {
    "components": dict(min_component_faces=0, keep_largest=None),
    "fill": dict(fill_holes=0, fill_bowties=False),
    "smooth": dict(smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, smooth_boundary="fixed"),
    "simplify": dict(simplify_cell=0.0, simplify_position="quadric"),
    "decimate": dict(decimate_faces=None, decimate_ratio=None, decimate_error=None),
}
DEFAULTS = {name: default for stage in OPTIONS.values() for name, default in stage.items()}

# option -> (key of tsdf_global, its type, given in voxel sizes): SlamSystem.extract_mesh's defaults
CONFIG = {
    "min_component_faces": ("mesh_min_component_faces", int, False),
    "simplify_cell": ("mesh_simplify_voxels", float, True),
    "smooth_iterations": ("mesh_smooth_iterations", int, False),
    "fill_holes": ("mesh_fill_holes", int, False),
    "fill_bowties": ("mesh_fill_bowties", bool, False),
    "decimate_faces": ("mesh_decimate_faces", int, False),
    "decimate_error": ("mesh_decimate_error", float, True),
}


def chain_options(options, what):
    """The keywords a caller gave as `**chain` -> the dict of those that do something: every option of a stage that is
    on, none of a stage that is off (fill_bowties only when True, the decimate_* each on its own: not None and not
    <= 0).  Handing the result on, or through here again, changes nothing.  A name that is no option raises the
    TypeError a def would; a fill_bowties that is not a bool (numpy's too) raises ValueError, fill on or off."""
    for name in options:
        if name not in DEFAULTS:
            raise TypeError(f"{what}() got an unexpected keyword argument {name!r}")
    o = dict(DEFAULTS, **options)
    o["fill_bowties"] = _bool_arg(o["fill_bowties"], "fill_bowties", what)
    on = {
        "components": o["min_component_faces"] > 0 or o["keep_largest"] is not None,
        "fill": o["fill_holes"] is not None and o["fill_holes"] > 0,
        "smooth": o["smooth_iterations"] is not None and o["smooth_iterations"] > 0,
        "simplify": o["simplify_cell"] is not None and o["simplify_cell"] > 0,
    }
    out = {name: o[name] for stage, is_on in on.items() if is_on for name in OPTIONS[stage]}
    if not out.get("fill_bowties"):
        out.pop("fill_bowties", None)
    out.update({name: o[name] for name in OPTIONS["decimate"] if o[name] is not None and not o[name] <= 0})
    return out


def config_defaults(options, cfg, voxel_size):
    """`options` with every option of CONFIG that is absent or None taken from `cfg` (tsdf_global).  Anything else, an
    explicit 0 included, stays as given."""
    options = dict(options)
    for name, (key, kind, in_voxels) in CONFIG.items():
        if options.get(name) is None:
            value = kind(cfg.get(key, 0))
            options[name] = value * float(voxel_size) if in_voxels else value
    return options


def run_chain(mesh, on):
    """The stages on `mesh` = (vertices, normals, faces[, colors]), `on` as chain_options returns it.  A stage that is off
    returns `mesh` itself."""
    o = dict(DEFAULTS, **on)
    mesh = filter_mesh(mesh, o["min_component_faces"], o["keep_largest"], _validate=False)
    mesh = fill_holes(mesh, o["fill_holes"], bowties=o["fill_bowties"])
    mesh = smooth_mesh(mesh, o["smooth_iterations"], o["smooth_lambda"], o["smooth_mu"], o["smooth_boundary"])
    mesh = simplify_mesh(mesh, o["simplify_cell"], o["simplify_position"])
    if any(name in on for name in OPTIONS["decimate"]):
        mesh = decimate_mesh(mesh, o["decimate_faces"], o["decimate_ratio"], o["decimate_error"], _validate=False)
    return mesh
