"""CPU-only: the C-ABI library builds/loads, exports every symbol the two headers (include/mvsnerf_hip.h = the stable tier,
include/mvsnerf_hip_internal.h = the internal one) declare, the stable tier is the frozen list below, and the ctypes table binds exactly that set.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import subprocess

from mvsnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_in(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mvsnerf_[a-z0-9_]+)\s*\(", src)))


def _declared():
    """every export = the stable tier (mvsnerf_hip.h) + the internal tier (mvsnerf_hip_internal.h)"""
    return sorted(set(_declared_in("mvsnerf_hip.h")) | set(_declared_in("mvsnerf_hip_internal.h")))


# The STABLE tier, frozen at ABI 12: the stage-level surface of SURVEY.md 8(b).  Adding, removing or re-typing an entry of this list is an
# ABI bump; the internal tier (per-shape kernels, *_tiles / *_parts / *_packed_elems queries, layout variants) may change freely.
STABLE_ABI_12 = """
abi_version ncdhw_to_ndhwc ndhwc_to_ncdhw nchw_to_nhwc resize_bilinear
planesweep_costvar_fwd planesweep_costvar_bwd planesweep_costvar_bwd_det_workspace_words planesweep_costvar_bwd_det homo_warp_fwd
conv3d_pack_weights conv3d_fwd conv_transpose3d_fwd abn_workspace_floats abn_stats abn_apply_add abn_apply_add_hwdc abn_bwd
conv3d_wgrad_workspace_floats conv3d_wgrad conv2d_pack_weights conv2d_fwd conv2d_wgrad_workspace_floats conv2d_wgrad channel_sum_workspace_floats channel_sum
raygen_fwd raygen_train_fwd volume_sample_fwd volume_sample_bwd volume_sample_bwd_det_workspace_words volume_sample_bwd_det color_sample_fwd color_feat_sample_fwd dir_feature_fwd gather_fwd posenc_fwd
mlp_packed_floats mlp_pack mlp_fwd mlp_packed_bf16_elems mlp_pack_bf16 mlp_fwd_bf16 mlp_fwd_bf16_train mlp_packed_bwd_bf16_elems mlp_pack_bwd_bf16 mlp_bwd_bf16
mlp_saved_floats mlp_gradslot_floats mlp_packed_bwd_floats mlp_bwd_workspace_floats mlp_pack_bwd mlp_fwd_train mlp_bwd
mlp_packed_split_elems mlp_pack_split mlp_fwd_split mlp_fwd_guarded
composite_fwd composite_bwd raymarch_fwd raymarch_fwd_batched raymarch_train_fwd raymarch_bwd render_workspace_floats render_pixels_fwd
adam_step_multi sample_pdf_fwd ray_marcher_fine_fwd ray_points_fwd
""".split()


def test_stable_tier_is_frozen():
    stable = _declared_in("mvsnerf_hip.h")
    assert stable == sorted("mvsnerf_" + n for n in STABLE_ABI_12), sorted(set(stable) ^ {"mvsnerf_" + n for n in STABLE_ABI_12})
    internal = _declared_in("mvsnerf_hip_internal.h")
    assert not set(stable) & set(internal)                       # an entry lives in exactly one tier
    # the stable header stands alone (a maintainer includes only it); the internal one pulls it in
    for h in ("mvsnerf_hip.h", "mvsnerf_hip_internal.h"):
        r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", h)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert "mvsnerf_hip_internal.h" not in open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read().split("*/", 1)[1]


def test_library_builds_and_exports_header_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = _declared()
    assert len(names) >= 20
    l = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(l, n)]
    assert not missing, f"declared in the header but not exported: {missing}"
    assert sorted(_lib.SIGNATURES) == names, (set(names) ^ set(_lib.SIGNATURES))
    assert _lib.lib().mvsnerf_abi_version() == 12
    # the dynamic symbol table is the header and nothing else (csrc/exports.map): no kernel host stubs, no C++-mangled helpers, no
    # A/B switches or diagnostics state
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exp_names = sorted(ln.split()[-1] for ln in exported.splitlines() if ln.strip())
    assert exp_names == names, sorted(set(exp_names) ^ set(names))[:10]
    # pure host-side queries work without a GPU
    # 32-point layout (12 feature k-steps x 4 blocks x 64 lanes, ...)
    n32 = 12 * 256 + 8192 * 2 + 16384 * 6 + 68 * 128 + 1416
    assert _lib.lib().mvsnerf_mlp_packed_floats(20) == n32
    assert _lib.lib().mvsnerf_mlp_packed_floats(21) == 0


def test_render_workspace_sizes():
    """The float counts of the two whole-frame workspaces: blocks pts, ndc (3P each), z (P), coarse z (B*S, importance sampling only), feat (F*P),
    raw (4P), rays_dir and dirs (3B each), every block rounded up to 16 bytes; P = B * (S + NI), and render_pixels is NI = 0, F = 8 + 4V."""
    lib = _lib.lib()
    r4 = lambda n: (n + 3) // 4 * 4
    for B in (1, 3, 512):
        for S in (1, 5, 128):
            for V in (1, 3, 8):
                F = 8 + 4 * V
                assert lib.mvsnerf_render_workspace_floats(B, S, V) == 2 * r4(3 * B * S) + r4(B * S) + r4(F * B * S) + r4(4 * B * S) + 2 * r4(3 * B)
                for NI in (0, 3):
                    P = B * (S + NI)
                    assert lib.mvsnerf_render_rays_workspace_floats(B, S, NI, F) == (2 * r4(3 * P) + r4(P) + (r4(B * S) if NI > 0 else 0) + r4(F * P)
                                                                                     + r4(4 * P) + 2 * r4(3 * B)), (B, S, NI, F)
    for bad in ((0, 5, 3), (3, 0, 3), (3, 5, 0), (-1, 5, 3)):
        assert lib.mvsnerf_render_workspace_floats(*bad) == 0, bad
    for bad in ((0, 5, 0, 20), (3, 0, 0, 20), (3, 5, -1, 20), (3, 5, 0, 8), (3, 5, 0, 22), (3, 5, 3, 18)):
        assert lib.mvsnerf_render_rays_workspace_floats(*bad) == 0, bad


def test_only_gfx950_code_objects():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", f"--input={_lib.LIB_PATH}"],
                         capture_output=True, text=True).stdout
    if out.strip():
        assert "gfx950" in out and not re.search(r"gfx9(0[0-9a]|4[0-9])\b", out)


def test_product_path_does_not_import_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "mvsnerf_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), f"{f} mentions the oracle"


def test_cross_file_helpers_are_declared_in_headers_only():
    """An internal helper (`mvs_*`) that one csrc file defines and another calls is declared once, in a header both include (conv.h, march.h), so the compiler
    checks definition and call against one prototype, default arguments included.  No .hip file may carry a prototype of its own: a declaration is a return
    type, an mvs_ name, a parameter list and `);` with no body (one line or several).  knobs.h, the constants that were all 1, stays gone."""
    csrc = os.path.join(ROOT, "mvsnerf_amd", "csrc")
    decl = re.compile(r"^[ \t]*(?:(?:static|inline|extern|const|unsigned)\s+)*(?!return\b|else\b)[A-Za-z_]\w*(?:\s*[*&])*\s+[*&]?(mvs_\w+)\s*\([^;{}]*\)\s*;", re.M)
    sources = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(sources) > 30 and "conv3d.hip" in sources and "encoder.hip" not in sources
    found = [(f, m.group(1)) for f in sources for m in decl.finditer(open(os.path.join(csrc, f)).read())]
    assert not found, f"prototypes of internal helpers outside the headers: {found}"
    assert decl.search("int mvs_x(const float* a,\n          int b = 0);") and not decl.search("    return mvs_x(a, b);\nint mvs_x(int a) { return a; }")
    assert not os.path.exists(os.path.join(csrc, "knobs.h"))


def test_plane_sweep_code_object_has_no_packed_fp32_arithmetic():
    """csrc/planesweep.hip must be built without packed fp32 instructions: next to 16-bit MFMA waves of another stream or process they computed wrong lanes
    (tests/test_gpu_costream.py is the GPU side).  The Makefile carries the flag and greps the code object; this compiles the file to ISA with
    the Makefile's own flags (hipcc cross-compiles without a GPU) and looks again."""
    csrc = os.path.join(ROOT, "mvsnerf_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule = mk[mk.index("build/planesweep.o:"):]
    assert "-fno-slp-vectorize" in rule.split("\n\n")[0], "the plane sweep's build rule lost -fno-slp-vectorize"
    flags = re.search(r"^FLAGS\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = os.path.join(csrc, "build", "planesweep_check.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-fno-slp-vectorize", "-S", "--cuda-device-only",
                        os.path.join(csrc, "planesweep.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    os.remove(out)
    assert "planesweep_kernel" in isa and "planesweep_if_kernel" in isa
    packed = re.findall(r"\bv_pk_\w+_f32\b", isa)
    assert not packed, f"{len(packed)} packed fp32 instructions in the plane sweep's code object: {sorted(set(packed))}"


def test_no_code_object_selects_the_high_half_of_src1_in_packed_fp32():
    """`v_pk_{fma,mul,add}_f32 ... op_sel:[x,1...]` (src1's high half feeding the low result) is the packed fp32 form that returned wrong values in lanes
    48-63 next to the fp16x3 conv0 of another stream (scratch/keep/pk_probe.hip, profiles/r05_pk_fma_opsel_reproducer.txt); the compiler picks the form, so
    the shipped bits are disassembled: csrc/check_isa.sh, which the Makefile also runs after linking."""
    csrc = os.path.join(ROOT, "mvsnerf_amd", "csrc")
    assert "check_isa.sh $@" in open(os.path.join(csrc, "Makefile")).read(), "the link rule lost its ISA check"
    r = subprocess.run(["sh", os.path.join(csrc, "check_isa.sh"), _lib.LIB_PATH, os.path.join(csrc, "build", "isa_test")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    n = int(re.search(r"check_isa: (\d+) code objects", r.stdout).group(1))
    assert n >= 18, r.stdout


def test_isa_check_rejects_a_library_that_holds_the_form(tmp_path):
    """The checker itself: a ten-line kernel with `v_pk_fma_f32 ... op_sel:[0,1,0]` (inline asm) linked into a shared object must fail check_isa.sh with the
    kernel's name in the report; the same kernel with the select on src0 must pass."""
    csrc = os.path.join(ROOT, "mvsnerf_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for sel, want_rc in (("op_sel:[0,1,0]", 1), ("op_sel:[1,0,0]", 0)):
        src = tmp_path / f"k{want_rc}.hip"
        src.write_text('#include <hip/hip_runtime.h>\n'
                       'typedef float f32x2 __attribute__((ext_vector_type(2)));\n'
                       '__global__ void isa_check_probe_kernel(f32x2* p) {\n'
                       '    f32x2 a = p[threadIdx.x], b = p[threadIdx.x + 64], c = p[threadIdx.x + 128];\n'
                       f'    asm volatile("v_pk_fma_f32 %0, %1, %2, %3 {sel}" : "=v"(c) : "v"(a), "v"(b), "v"(c));\n'
                       '    p[threadIdx.x] = c;\n'
                       '}\n')
        lib = tmp_path / f"libk{want_rc}.so"
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", str(src), "-o", str(lib)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(["sh", os.path.join(csrc, "check_isa.sh"), str(lib), str(tmp_path / f"isa{want_rc}")], capture_output=True, text=True)
        assert r.returncode == want_rc, r.stdout + r.stderr
        if want_rc:
            assert "isa_check_probe_kernel" in r.stdout and "1 packed fp32 instruction" in r.stdout, r.stdout
