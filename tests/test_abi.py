"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares; mslam_hip.py takes every ctypes signature from that header (there is no table of its own), and the
Python side raises (never falls back) without a device."""
import ctypes
import os
import re

import pytest
import torch

import mslam_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mslam_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(mslam_hip.LIB_PATH), "build libmslam_hip.so first (__graft_entry__.build())"
    handle = ctypes.CDLL(mslam_hip.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 5
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in include/mslam_hip.h but not exported"


def _header_declarations():
    """An independent second reading of the header: {name: (return type text, parameter count)}."""
    text = open(os.path.join(ROOT, "include", "mslam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t*]*?)\s*\b(mslam_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        decls[name] = (" ".join(ret.split()), 0 if params in ("", "void") else params.count(",") + 1)
    return decls


def test_binding_table_matches_header():
    assert sorted(mslam_hip.exported_symbols()) == _header_symbols()
    decls = _header_declarations()
    assert sorted(decls) == _header_symbols()
    handle = mslam_hip.lib()
    for name, (ret, n_params) in decls.items():
        fn = getattr(handle, name)
        assert len(fn.argtypes) == n_params, name
        assert (fn.restype is ctypes.c_size_t) == (ret == "size_t"), name
        assert (fn.restype is ctypes.c_char_p) == (name == "mslam_last_error"), name
        if ret != "size_t" and name != "mslam_last_error":
            assert fn.restype is ctypes.c_int, name


def test_pinned_signatures():
    """Full argtypes / restype of a sample that covers every type the binding knows, spelled out by hand."""
    vp, i, f, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    u64, u32, i64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
    pinned = {
        "mslam_sim3_act": (i, [vp] * 3 + [i, ctypes.c_longlong, i, vp]),
        "mslam_tsdf_dump": (i, [vp, u64, vp, vp, vp, u32, vp]),
        "mslam_tsdf_mesh_emit": (i, [vp, u64] + [d] * 3 + [vp] * 5 + [sz] + [vp] * 3 + [i64, i64, vp]),
        "mslam_track_pose": (i, [i] + [vp] * 6 + [i, vp, i, i] + [f] * 3 + [i, f, i, i, f, f, vp, vp, sz, vp]),
        "mslam_mast3r_create": (i, [vp, vp, vp, vp, i, vp]),
        "mslam_gn_workspace_bytes": (sz, [i] * 4),
        "mslam_tsdf_integrate_workspace_bytes": (sz, [i, d, d, d]),
        "mslam_last_error": (ctypes.c_char_p, []),
        "mslam_abi_version": (i, []),
    }
    handle = mslam_hip.lib()
    for name, (restype, argtypes) in pinned.items():
        fn = getattr(handle, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name


def test_parse_header_rejects_what_it_does_not_know():
    with pytest.raises(ValueError, match=r"mslam_bad.*short"):
        mslam_hip.parse_header("int mslam_bad(void* p, short n);")
    with pytest.raises(ValueError, match=r"mslam_bad.*struct box b"):
        mslam_hip.parse_header("int mslam_bad(struct box b, void* stream);")
    with pytest.raises(ValueError, match=r"mslam_bad.*cb"):
        mslam_hip.parse_header("int mslam_bad(void (*cb)(int), void* stream);")
    with pytest.raises(ValueError, match=r"mslam_bad.*float v\[3\]"):
        mslam_hip.parse_header("int mslam_bad(float v[3], void* stream);")
    with pytest.raises(ValueError, match=r"mslam_bad.*float"):
        mslam_hip.parse_header("float mslam_bad(int n);")
    with pytest.raises(ValueError):
        mslam_hip.parse_header("int mslam_ok(int n);\ntypedef int mslam_t;")


def test_parse_header_reads_plain_declarations():
    text = """
    /* int mslam_fake(int); */
    // int mslam_fake2(int n);
    #define MSLAM_OK 0
    #ifdef __cplusplus
    extern "C" {
    #endif
    const char* mslam_msg(void);
    size_t mslam_bytes();
    int mslam_split(const float* a,   /* size_t mslam_fake3(void); */
                    const int n, double const x,
                    void* const* pp, long long k,
                    uint64_t c, uint32_t m, int64_t v, size_t b, float e,
                    void** out);
    #ifdef __cplusplus
    }
    #endif
    """
    vp = ctypes.c_void_p
    assert mslam_hip.parse_header(text) == {
        "mslam_msg": (ctypes.c_char_p, []),
        "mslam_bytes": (ctypes.c_size_t, []),
        "mslam_split": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_double, vp, ctypes.c_longlong, ctypes.c_uint64,
                                       ctypes.c_uint32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, vp]),
    }


def test_header_constants():
    """header_constants() reads the integer #defines of the real header; the literals here are the independent
    statement."""
    c = mslam_hip.header_constants()
    want = {"MSLAM_MESH_ALIGN_STATE_BYTES": 72, "MSLAM_MESH_ALIGN_LOG_DOUBLES": 24, "MSLAM_MESH_ALIGN_OK": 0,
            "MSLAM_MESH_ALIGN_DEGENERATE": 1, "MSLAM_OK": 0, "MSLAM_EINVAL": -1, "MSLAM_EHIP": -2, "MSLAM_ENOMEM": -3,
            "MSLAM_ENODEV": -4}
    assert {k: c.get(k) for k in want} == want
    with open(os.path.join(ROOT, "include", "mslam_hip.h")) as f:
        header = f.read()
    for name, value in want.items():                       # the header's values, read without the parser
        m = re.search(rf"^#define {name} \(?(-?\d+)\)?", header, flags=re.M)
        assert m is not None and int(m.group(1)) == value, name
    assert "MSLAM_HIP_H" not in c                           # the include guard has no value
    text = """
#define MSLAM_A 7   /* a comment */
#define MSLAM_B (-12)  // another
  #  define MSLAM_C ( - 3 )
#define MSLAM_RATIO 1.5
#define MSLAM_HALF 0.5f
#define MSLAM_SUM (1 + 2)
#define MSLAM_HEX 0x10
#define MSLAM_NAME "text"
#define MSLAM_OTHER MSLAM_A
#define MSLAM_F(x) 3
#define MSLAM_EMPTY
#define OTHER_D 4
/* #define MSLAM_COMMENTED 9 */
"""
    assert mslam_hip.header_constants(text) == {"MSLAM_A": 7, "MSLAM_B": -12, "MSLAM_C": -3}


def test_abi_version():
    assert mslam_hip.lib().mslam_abi_version() >= 1


def test_no_cpu_fallback():
    import mast3r_slam_backends as be

    rays = torch.zeros(1, 4, 4, 9)
    pts = torch.zeros(1, 16, 3)
    p0 = torch.zeros(1, 16, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        be.iter_proj(rays, pts, p0, 10, 1e-8, 1e-6)


def test_contiguity_error_matches_reference_wording():
    import mast3r_slam_backends as be

    rays = torch.zeros(1, 4, 9, 4).permute(0, 1, 3, 2)
    with pytest.raises(RuntimeError, match="rays_img_with_grad must be contiguous"):
        be.iter_proj(rays, torch.zeros(1, 16, 3), torch.zeros(1, 16, 2), 10, 1e-8, 1e-6)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
                assert "liboracle" not in src, f
