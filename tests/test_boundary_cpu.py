"""The drop-in boundary, guarded without a Rust toolchain (round 5's verdict, items 5 and 7).

INTEGRATION.md shows the `extern "C"` blocks and `#[repr(C)]` structs a pathtrace-rs maintainer would add around `Scene::new` /
`Scene::update` (scene.rs:73-79). Nothing in this image compiles Rust, so these tests keep that text honest against the things that DO
exist here: include/ptgpu.h (through a C program compiled with gcc: sizeof / offsetof of every struct field), the ctypes mirrors in
pathtrace-rs_amd/ptgpu.py, and the symbols libptgpu.so exports. CPU only; no compute calls.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ptgpu.h")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")
LIB = os.path.join(ROOT, "pathtrace-rs_amd", "_build", "libptgpu.so")


def _rust_blocks():
    text = open(INTEGRATION).read()
    return "\n".join(re.findall(r"```rust\n(.*?)```", text, flags=re.S))


def _strip_rust_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


# ---- Rust type -> (size, alignment) under #[repr(C)] on x86-64 -------------------------------------------------------------------
_PRIM = {"u8": (1, 1), "i8": (1, 1), "u16": (2, 2), "i16": (2, 2), "u32": (4, 4), "i32": (4, 4), "f32": (4, 4), "u64": (8, 8), "i64": (8, 8),
         "f64": (8, 8), "usize": (8, 8), "isize": (8, 8), "c_int": (4, 4), "c_char": (1, 1)}


def _rust_layout(ty, structs):
    ty = ty.strip()
    if ty.startswith("*const ") or ty.startswith("*mut "):
        return 8, 8
    m = re.fullmatch(r"\[(.+);\s*(\d+)\]", ty)
    if m:
        size, align = _rust_layout(m.group(1), structs)
        return size * int(m.group(2)), align
    if ty in _PRIM:
        return _PRIM[ty]
    if ty in structs:
        return structs[ty]["size"], structs[ty]["align"]
    raise AssertionError("INTEGRATION.md uses a Rust type this test cannot lay out: %r" % ty)


def _split_top_level(s, sep=","):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{<":
            depth += 1
        elif ch in ")]}>":
            depth -= 1
        if ch == sep and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return [x.strip() for x in out if x.strip()]


def _rust_structs():
    """name -> {fields: [(name, type, offset, size)], size, align} for every #[repr(C)] struct of INTEGRATION.md, in order of appearance."""
    src = _strip_rust_comments(_rust_blocks())
    structs = {}
    for name, body in re.findall(r"#\[repr\(C\)\]\s*pub struct (\w+)\s*\{(.*?)\}", src, flags=re.S):
        off, align, fields = 0, 1, []
        for f in _split_top_level(body):
            m = re.fullmatch(r"pub (\w+)\s*:\s*(.+)", f, flags=re.S)
            assert m, "unparsed field %r of %s" % (f, name)
            size, al = _rust_layout(m.group(2), structs)
            off = (off + al - 1) // al * al
            fields.append((m.group(1), " ".join(m.group(2).split()), off, size))
            off += size
            align = max(align, al)
        structs[name] = {"fields": fields, "size": (off + align - 1) // align * align, "align": align}
    return structs


def _c_layout(structs, tmp_path):
    """sizeof / offsetof of the same fields from include/ptgpu.h, through gcc."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ptgpu.h"', "int main(void) {"]
    for name, st in structs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (name, name))
        for fname, _ty, _off, _sz in st["fields"]:
            if name == "pt_camera":
                continue   # (Rust holds the 24 floats as one array: sizes are compared, the header's field order is camera.rs:8-19's)
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, fname, name, fname, name, fname))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {}
    for l in out.splitlines():
        parts = l.split()
        got[parts[0]] = tuple(int(x) for x in parts[1:] if x.isdigit())
    return got


_CTYPES = {"pt_params": "PtParams", "pt_camera": "PtCamera", "pt_sphere": "PtSphere", "pt_material": "PtMaterial", "pt_texture": "PtTexture",
           "pt_perlin": "PtPerlin", "pt_bvh_node": "PtBvhNode", "pt_scene_desc": "PtSceneDesc", "pt_hitable": "PtHitable", "pt_affine": "PtAffine",
           "pt_image": "PtImage", "pt_world_desc": "PtWorldDesc"}


def test_rust_structs_of_integration_md_match_the_header_and_the_ctypes_mirrors(ptgpu, tmp_path):
    """Every #[repr(C)] struct INTEGRATION.md shows has the size and the field offsets / widths of its namesake in include/ptgpu.h (gcc),
    and the ctypes Structure that bench.py and the tests really call the library with agrees with both -- so a field added to the header
    without its Rust line (or the other way round) fails here, on the CPU, instead of corrupting a frame on somebody's GPU."""
    structs = _rust_structs()
    assert {"pt_params", "pt_camera", "pt_sphere", "pt_material", "pt_texture", "pt_perlin", "pt_bvh_node", "pt_scene_desc", "pt_hitable", "pt_affine",
            "pt_image", "pt_node", "pt_world_desc"} <= set(structs), sorted(structs)
    c = _c_layout(structs, tmp_path)
    for name, st in structs.items():
        assert c[name] == (st["size"],), "%s: Rust text lays out %d bytes, the header %r" % (name, st["size"], c[name])
        for fname, ty, off, size in st["fields"]:
            if name == "pt_camera":
                continue
            assert c["%s.%s" % (name, fname)] == (off, size), "%s.%s (%s): Rust text offset %d size %d, header %r" % (name, fname, ty, off, size, c["%s.%s" % (name, fname)])
        mirror = getattr(ptgpu, _CTYPES[name], None) if name in _CTYPES else None
        if mirror is None:
            continue
        assert C.sizeof(mirror) == st["size"], "%s: ctypes mirror %d bytes, Rust text / header %d" % (name, C.sizeof(mirror), st["size"])
        if name == "pt_camera":
            continue
        by_name = {f[0]: getattr(mirror, f[0]) for f in mirror._fields_}
        for fname, ty, off, size in st["fields"]:
            # (the mirrors name the same fields; a renamed one fails the lookup)
            assert fname in by_name, "%s: ctypes mirror has no field %r (it has %s)" % (name, fname, sorted(by_name))
            assert (by_name[fname].offset, by_name[fname].size) == (off, size), "%s.%s: ctypes %r, header (%d, %d)" % (name, fname, (by_name[fname].offset, by_name[fname].size), off, size)
    # pt_camera: 24 floats in camera.rs:8-19's order on all three sides
    cam = open(HEADER).read()
    m = re.search(r"typedef struct pt_camera \{(.*?)\} pt_camera;", cam, flags=re.S)
    assert m
    order = re.findall(r"\b(origin|lower_left_corner|horizontal|vertical|u|v|w|time0|time1|lens_radius)\b\s*(?:\[3\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert order == ["origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w", "time0", "time1", "lens_radius"], order
    assert [f[0] for f in ptgpu.PtCamera._fields_] == order


def _c_prototypes():
    """name -> parameter count, for every function include/ptgpu.h declares."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\b(pt_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = " ".join(args.split())
        protos[name] = 0 if args in ("", "void") else len(_split_top_level(args))
    return protos


def _rust_externs():
    """name -> parameter count, for every `pub fn` inside an extern "C" block of INTEGRATION.md."""
    src = _strip_rust_comments(_rust_blocks())
    fns = {}
    for block in re.findall(r'extern "C"\s*\{(.*?)\n\}', src, flags=re.S) + re.findall(r'extern "C"\s*\{([^\n]*)\}', src):
        for name, args in re.findall(r"pub fn (pt_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->[^;]+)?;", block, flags=re.S):
            fns[name] = len(_split_top_level(" ".join(args.split())))
    return fns


def test_every_exported_symbol_is_declared_and_either_bound_or_named_as_diagnostics():
    """`nm -D libptgpu.so`: every pt_* symbol the shared object exports is declared in include/ptgpu.h and is either bound in one of
    INTEGRATION.md's extern "C" blocks -- with the header's parameter count -- or named in its list of entry points a host does not bind.
    And nothing is bound or declared that the library does not export."""
    if not os.path.exists(LIB):
        pytest.skip("libptgpu.so not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pt_[a-z0-9_]+)$", nm, flags=re.M))
    assert len(exported) >= 40, sorted(exported)
    protos, bound = _c_prototypes(), _rust_externs()
    assert exported == set(protos), "declared but not exported: %s; exported but not declared: %s" % (sorted(set(protos) - exported), sorted(exported - set(protos)))
    text = open(INTEGRATION).read()
    m = re.search(r"\*\*Entry points a host does not bind\*\*(.*?)\n\n", text, flags=re.S)
    assert m, "INTEGRATION.md lost its list of unbound entry points"
    diagnostics = set(re.findall(r"`(pt_[a-z0-9_]+)`", m.group(1)))
    assert not (diagnostics & set(bound)), sorted(diagnostics & set(bound))
    assert exported == set(bound) | diagnostics, "neither bound nor listed: %s; bound / listed but not exported: %s" % (
        sorted(exported - set(bound) - diagnostics), sorted((set(bound) | diagnostics) - exported))
    wrong = {n: (bound[n], protos[n]) for n in bound if bound[n] != protos[n]}
    assert not wrong, "parameter counts (INTEGRATION.md, header): %s" % wrong
    # the seam itself (scene.rs:73-79): Scene::new -> pt_scene_create[_world], Scene::update -> pt_render, Drop -> pt_scene_destroy
    assert {"pt_scene_create", "pt_scene_create_world", "pt_render", "pt_scene_destroy", "pt_last_error"} <= set(bound)


def test_a_second_hip_runtime_in_the_process_is_reported_not_guessed(ptgpu):
    """PyTorch ships its own libamdhip64; libptgpu.so links the system's. Two HIP runtimes in one process only work when torch's initialises
    first (tests/conftest.py), and the failure the other way round is a confusing "no HIP GPUs". ptgpu.hip_runtimes_mapped() lists the copies
    mapped into this process and ptgpu.check_hip_runtimes() raises a clear error for the order that cannot work."""
    maps = ptgpu.hip_runtimes_mapped()
    assert isinstance(maps, list) and all(os.path.basename(p).startswith("libamdhip64") for p in maps)
    # the decision itself, on made-up inputs: one runtime is always fine; two are fine only when torch's had initialised before ours loaded
    ok = ptgpu._hip_runtime_conflict
    assert ok(["/opt/rocm/lib/libamdhip64.so.7"], torch_initialised=False) is None
    assert ok(["/opt/rocm/lib/libamdhip64.so.7", "/usr/lib/python3/dist-packages/torch/lib/libamdhip64.so"], torch_initialised=True) is None
    msg = ok(["/opt/rocm/lib/libamdhip64.so.7", "/usr/lib/python3/dist-packages/torch/lib/libamdhip64.so"], torch_initialised=False)
    assert msg and "import torch" in msg and "torch.cuda.init()" in msg and "libamdhip64" in msg


# ---- the pin kit stays turnkey (tools/pin_against_rust.py + tools/pin/offline_dump_f32.patch) -----------------------------------------
def test_pin_kit_runs_without_cargo_and_its_patch_still_applies(tmp_path):
    """Parity with the Rust binary is unpinned until someone with cargo runs ONE command (README "Pinning the oracle"). What can rot meanwhile
    is checked here: the script starts and explains itself without cargo, its PNG reader decodes what the product's writer encodes, the
    expectations file holds the ten frames, and the 10-line patch that makes the reference dump its raw f32 frame still applies: to the
    pre-image it carries itself, and to a reference checkout as well where PT_REFERENCE_TREE names one."""
    tool = os.path.join(ROOT, "tools", "pin_against_rust.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "cargo" in out.stdout.lower(), out.stdout + out.stderr
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("pin_against_rust", tool)
    pin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pin)
    exp = json.load(open(os.path.join(ROOT, "tests", "golden", "rust_expectations.json")))
    assert len(exp["cases"]) >= 10 and exp.get("status")
    # the PNG reader against a PNG this repo's own writer produced (host/offline.cpp through the CLI is exercised in test_host_cpu; here: zlib + filters)
    import zlib
    import struct
    import numpy as np
    rgb = (np.arange(7 * 5 * 3, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(5, 7, 3)
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(5))
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
    f = tmp_path / "t.png"
    f.write_bytes(png)
    got = pin.png_rgb8(str(f))
    assert np.array_equal(np.frombuffer(got, np.uint8).reshape(5, 7, 3), rgb)
    patch = os.path.join(ROOT, "tools", "pin", "offline_dump_f32.patch")
    assert os.path.exists(patch)
    # The reference tree is not part of this repository: the file the patch edits is rebuilt from the patch's own pre-image (context and
    # removed lines at the line numbers its hunk headers name, blank lines elsewhere). The patch must apply to that file cleanly and leave
    # exactly its post-image there, so an edit that breaks a hunk's counts, offsets or context is caught without the reference.
    text = open(patch).read()
    target = re.search(r"^\+\+\+ b/(\S+)$", text, flags=re.M).group(1)
    hunks = re.findall(r"^@@ -(\d+),(\d+) \+(\d+),(\d+) @@[^\n]*\n((?:[ +-][^\n]*\n?)*)", text, flags=re.M)
    assert target == "src/offline.rs" and hunks, text[:200]
    before, after = [], {}
    for old_start, old_len, new_start, new_len, body in hunks:
        lines = body.splitlines()
        old = [l[1:] for l in lines if l[:1] in " -"]
        new = [l[1:] for l in lines if l[:1] in " +"]
        assert (len(old), len(new)) == (int(old_len), int(new_len)), "hunk @@ -%s,%s +%s,%s @@ miscounts its lines" % (old_start, old_len, new_start, new_len)
        before += [""] * (int(old_start) - 1 - len(before)) + old
        after[int(new_start)] = new
    src = tmp_path / "pre" / target
    src.parent.mkdir(parents=True)
    src.write_text("\n".join(before) + "\n")
    chk = subprocess.run(["git", "apply", "--verbose", patch], cwd=tmp_path / "pre", capture_output=True, text=True)
    assert chk.returncode == 0, chk.stdout + chk.stderr
    got = src.read_text().splitlines()
    for start, new in after.items():
        assert got[start - 1:start - 1 + len(new)] == new
    assert any("PT_DUMP_F32" in l for l in got)
    # where a checkout of the reference is at hand, the patch is also checked against it (PT_REFERENCE_TREE=<checkout>)
    ref = os.environ.get("PT_REFERENCE_TREE")
    if ref:
        copy = tmp_path / "ref"
        shutil.copytree(ref, copy, ignore=shutil.ignore_patterns("target", ".git"))
        chk = subprocess.run(["git", "apply", "--check", "--verbose", patch], cwd=copy, capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout + chk.stderr
