"""C-ABI checks that need no GPU: libseer_hip.so builds for gfx950, loads, and exports every symbol that
include/seer_hip.h declares; the ctypes binding covers exactly that set; the product has no CPU fallback."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "seer_hip.h"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(seer_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    from seervideoldm_amd.build import build_library
    return build_library()


def test_library_exports_every_declared_symbol(lib_path):
    names = _declared()
    assert len(names) >= 20
    lib = ctypes.CDLL(str(lib_path))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in seer_hip.h but not exported"


def test_binding_matches_header(lib_path):
    from seervideoldm_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    lib = _lib.load()
    assert lib.seer_abi_version() == _lib.ABI_VERSION
    assert lib.seer_build_arch() == b"gfx950"
    assert b"invalid" in lib.seer_strerror(-22)


def test_one_entry_point_per_kernel(lib_path):
    """no `_dt` / `_pre` twin is declared, none of the sampler step's `_dev` / `_rng` twins of ABI <= 26 either, and the library
    exports no seer_* symbol beyond the header's: the forwarders of ABI <= 25 are gone, not merely undeclared"""
    import subprocess
    names = _declared()
    assert not [n for n in names if n.endswith(("_dt", "_pre"))]
    assert not set(names) & {"seer_cfg_ddim_step_dev", "seer_cfg_ddim_step_rng", "seer_cfg_ddim_step_rng_dev",
                             "seer_cfg_ddim_invert_step_dev", "seer_cfg_dpm_step_dev", "seer_v_to_eps_dev", "seer_slot_plms_step_begin",
                             "seer_slot_cfg_ddim_step_rng"}
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True, check=True).stdout
    exported = sorted({l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("seer_")})
    assert exported == names


STRUCTS = {"seer_gemm_desc": "GemmDesc", "seer_attn_desc": "AttnDesc", "seer_attn_bwd_desc": "AttnBwdDesc",
           "seer_rowchain_desc": "RowChainDesc", "seer_tn_item": "TnItem", "seer_colfinal_item": "ColfinalItem",
           "seer_transpose_item": "TransposeItem"}


def test_struct_layout_matches_the_compiler(tmp_path):
    """all seven structs: field names and order == the header's (read here by a parser of the test's own), and sizeof, every
    field's offset and size == what gcc makes of the header (a C program generated from the classes prints them)"""
    import subprocess
    from seervideoldm_amd import _lib
    text = HEADER.read_text()
    assert _lib.CLASS_NAMES == STRUCTS and len(re.findall(r"typedef struct", text)) == len(STRUCTS)
    lines, want = [], {}
    for cname, pyname in STRUCTS.items():
        cls = getattr(_lib, pyname)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            names = stmt.split(None, 1)[1] if not stmt.startswith("const") else stmt.split(None, 2)[2]
            for nm in names.split(","):
                fields.append(nm.strip().lstrip("*").strip())
        assert fields == [f[0] for f in cls._fields_], cname
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = ctypes.sizeof(cls)
        for f in fields:
            lines.append(f'    printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
            want[f"{cname}.{f}"] = (getattr(cls, f).offset, getattr(cls, f).size)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "seer_hip.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n    return 0;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-O1", f"-I{HEADER.parent}", str(src), "-o", str(tmp_path / "layout")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    got = {}
    for l in out.splitlines():
        key, *nums = l.split()
        got[key] = int(nums[0]) if len(nums) == 1 else (int(nums[0]), int(nums[1]))
    assert got == want and got["seer_transpose_item"] == 56


GOOD = """#define SEER_FLAG 4u
typedef struct seer_d { const void* p; int32_t a, b; double c; } seer_d;
const char* seer_name(int code);
int32_t seer_f(const seer_d* d /* host */, const float* x, int32_t out[5] /* host */, int64_t n[2], uint64_t s, void* stream);
"""


def test_parser_types_of_a_well_formed_header():
    from seervideoldm_amd._lib import parse_header
    constants, structs, sigs = parse_header(GOOD)
    D = structs["seer_d"]
    assert constants == {"SEER_FLAG": 4} and list(structs) == ["seer_d"] and list(sigs) == ["seer_name", "seer_f"]
    assert D._fields_ == [("p", ctypes.c_void_p), ("a", ctypes.c_int32), ("b", ctypes.c_int32), ("c", ctypes.c_double)]
    assert sigs["seer_name"] == ([ctypes.c_int], ctypes.c_char_p)
    assert sigs["seer_f"] == ([ctypes.POINTER(D), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.c_void_p], ctypes.c_int32)
    assert parse_header(GOOD, {"seer_d": "Desc"})[1]["seer_d"].__name__ == "Desc"


@pytest.mark.parametrize("bad, line, says", [
    ("int seer_f(int32_t n, long m);", 3, "long m"),                                    # an unknown scalar type
    ("typedef struct seer_e { int32_t a; size_t n; } seer_e;", 3, "size_t n"),          # a struct field of unknown type
    ("static int seer_f(int32_t n);", 3, "static int seer_f"),                          # `seer_...(` that is no declaration
    ("int seer_f(int32_t n) { return seer_g(n); }", 3, "seer_g"),
    ("seer_d seer_f(int32_t n);", 3, "seer_d"),                                         # a struct by value is no scalar
    ("#define SEER_SCALE 1.5f", 3, "SEER_SCALE"),
], ids=["scalar", "field", "not-a-declaration", "body", "struct-by-value", "define"])
def test_parser_refuses_what_it_does_not_understand(bad, line, says):
    """a four-line header whose third line is not understood: SeerHipError with the line and its text, nothing skipped"""
    from seervideoldm_amd._lib import SeerHipError, parse_header
    lines = GOOD.splitlines()
    text = "\n".join(lines[:2] + [bad] + lines[2:3]) + "\n"
    parse_header("\n".join(lines[:2] + lines[2:3]) + "\n")                              # the same header without that line parses
    with pytest.raises(SeerHipError) as e:
        parse_header(text)
    assert f"line {line}:" in str(e.value) and says in str(e.value), str(e.value)


def test_transpose_items_pack_to_the_c_struct():
    """train_ops.pack_transpose_items == struct.pack of seer_transpose_item's fields (5 x int64, 4 x int32); the second item has
    cols and ldx close to 2^31: two int32 fields, not the two halves of one int64"""
    import struct
    from seervideoldm_amd import _lib
    from seervideoldm_amd.train_ops import pack_transpose_items
    a = dict(x=0x7F0000001000, y=0x7F0000200000, rows=3, ldy=64, tile0=0, cols=320, ldx=328, tiles_r=1)
    b = dict(x=0x7F0123456780, y=0x7FFFFFFFFFF0, rows=65528, ldy=65536, tile0=5, cols=65528, ldx=2 ** 31 - 8, tiles_r=1024)
    want = (struct.pack("<5q4i", 0x7F0000001000, 0x7F0000200000, 3, 64, 0, 320, 328, 1, 0)
            + struct.pack("<5q4i", 0x7F0123456780, 0x7FFFFFFFFFF0, 65528, 65536, 5, 65528, 2 ** 31 - 8, 1024, 0))
    assert ctypes.sizeof(_lib.TransposeItem) == 56 and len(want) == 112
    assert pack_transpose_items([a, b]) == want and pack_transpose_items([b]) == want[56:]


def test_argument_validation_without_gpu(lib_path):
    """entry points reject bad descriptors before touching the device (no compute calls here)."""
    from seervideoldm_amd import _lib
    lib = _lib.load()
    assert lib.seer_gemm_bf16(None, None) == -22
    d = _lib.GemmDesc()
    d.M, d.N, d.K = 128, 128, 100          # K not a multiple of 64
    d.A = d.W = d.C = 1
    assert lib.seer_gemm_bf16(ctypes.byref(d), None) == -22
    a = _lib.AttnDesc()
    a.Q = a.K = a.V = a.O = 1
    a.batch, a.heads, a.head_dim, a.Sq, a.Sk = 1, 8, 64, 16, 16     # head_dim 64 is not built
    assert lib.seer_attn_fwd(ctypes.byref(a), None) == -38
    r = _lib.RowChainDesc()
    assert lib.seer_rowchain_c320(None, None) == -22 and lib.seer_rowchain_c320(ctypes.byref(r), None) == -22
    r.inp = r.w1f = r.h = 16
    r.M, r.ld_in, r.ldh = 200, 320, 320
    r.gn_stats = r.gn_gamma = r.gn_beta = 16
    r.gn_count, r.groups, r.rows_per_batch = 500.0, 32, 50           # a 96-row tile would span three batch elements
    assert lib.seer_rowchain_c320(ctypes.byref(r), None) == -38
    # grouped training entries: host tables are checked item by item before anything is launched
    assert lib.seer_gemm_tn_grouped_f32(None, 0, None, 0, None) == -22 and lib.seer_colfinal_grouped(None, 0, None) == -22
    assert lib.seer_layernorm_bwd_slabs(0) == -22 and lib.seer_layernorm_bwd_slabs(100) == 13 and lib.seer_layernorm_bwd_slabs(10 ** 6) == 1024
    items = (_lib.TnItem * 2)()
    for it in items:
        it.A = it.B = it.C = 16
        it.lda, it.ldb, it.M, it.N, it.K = 320, 320, 4096, 320, 320
    assert lib.seer_gemm_tn_grouped_workspace_bytes(items, 2) == 0                  # unsplit up to 16 384 rows: no workspace
    items[1].M = 40000                                                           # three K slices of [N*K + N] floats
    assert lib.seer_gemm_tn_grouped_workspace_bytes(items, 2) == 3 * (320 * 320 + 320) * 4
    items[1].lda = 100                                                           # row pitch below N
    assert lib.seer_gemm_tn_grouped_workspace_bytes(items, 2) == -22 and lib.seer_gemm_tn_grouped_f32(items, 2, None, 0, None) == -22
    cf = (_lib.ColfinalItem * 1)()
    cf[0].ws, cf[0].nblocks, cf[0].NV, cf[0].C = 16, 4, 3, 320                     # NV is 1 or 2
    assert lib.seer_colfinal_grouped(cf, 1, None) == -22
    # every entry point with a storage type: a dtype that is neither SEER_DT_BF16 (0) nor SEER_DT_F16 (1) is -22 with otherwise
    # plausible arguments: 16 = an aligned non-NULL pointer, and shapes every entry point accepts, so that the dtype is the only
    # reason for the refusal (with a good dtype these calls would launch, which is why only the bad one is made here) ...
    P, bad = 16, 2
    assert lib.seer_groupnorm_stats(P, 320, None, 0, 1, 64, 32, P, P, bad, None) == -22
    assert lib.seer_groupnorm_apply(P, 320, None, 0, 1, 64, 32, P, 640.0, 1e-5, P, P, 0, P, bad, None) == -22
    assert lib.seer_groupnorm_apply_from_colsums(P, 320, None, 0, P, 1, 1, None, 0, 0, 1, 256, 32, 2560.0, 1e-5, P, P, 0, P, bad, None) == -22
    assert lib.seer_groupnorm_apply_fx(P, 320, None, 0, P, 1, None, 0, 1, 256, 32, 2560.0, 1e-5, P, P, 0, P, None, bad, None) == -22
    assert lib.seer_groupnorm_stats_fx(P, 320, 1, 256, P, bad, None) == -22
    assert lib.seer_layernorm(P, 4, 320, 320, P, P, 1e-5, P, 320, bad, None) == -22
    assert lib.seer_softmax_rows(P, 0, 4, 256, 256, 1.0, P, 256, bad, None) == -22
    assert lib.seer_linear_smallm(P, 2, 320, P, P, 1280, 0, 1, P, bad, None) == -22
    assert lib.seer_conv_in(P, 1, 4, 2, 8, 8, P, P, 320, P, bad, None) == -22
    assert lib.seer_conv_out(P, 1, 320, 2, 8, 8, P, P, 4, P, bad, None) == -22
    assert lib.seer_cast_f32(P, 1024, P, bad, None) == -22
    ff = (P, 320, P, 320, P, 320, 96, P, P, 1e-5, P, P, P, P, None, 0, 0, None)
    assert lib.seer_ff_fused_c320(P, 320, P, P, *ff, bad, None) == -22
    assert lib.seer_ff_fused_c320(None, 0, None, None, *ff, bad, None) == -22          # without the prologue
    # ... and it is refused ahead of the shape classes that are not built: -22, not -38; a good dtype gets the -38
    assert lib.seer_layernorm(P, 4, 2048, 2048, P, P, 1e-5, P, 2048, bad, None) == -22
    assert lib.seer_layernorm(P, 4, 2048, 2048, P, P, 1e-5, P, 2048, 1, None) == -38
    assert lib.seer_softmax_rows(P, 0, 4, 8192, 8192, 1.0, P, 8192, bad, None) == -22
    assert lib.seer_softmax_rows(P, 0, 4, 8192, 8192, 1.0, P, 8192, 0, None) == -38
    assert lib.seer_conv_out(P, 1, 320, 2, 8, 8, P, P, 4, P, 1, None) == -38           # fp16 conv_out exists for Cout = 3 only


def test_header_is_plain_c_and_the_c_caller_links(lib_path):
    """include/seer_hip.h compiles as C99 and tests/abi_caller.c (gcc, no C++, no Python) links against the library"""
    import subprocess
    from seervideoldm_amd.build import build_c_caller
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", str(HEADER)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = build_c_caller()
    assert exe.exists()
    syms = subprocess.run(["nm", "-D", "--undefined-only", str(exe)], capture_output=True, text=True).stdout
    assert "seer_gemm_bf16" in syms and "seer_attn_fwd" in syms


@pytest.mark.gpu
def test_c_caller_runs_on_the_gpu():
    """the C host calls seer_gemm_bf16 and seer_attn_fwd and checks them against its own arithmetic"""
    import subprocess
    from seervideoldm_amd.build import build_c_caller
    exe = build_c_caller()           # normally already built by __graft_entry__.build() and shipped with the snapshot
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ABI_CALLER_OK" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_no_cpu_fallback():
    from seervideoldm_amd import SeerUNet, _lib, ops
    with pytest.raises(_lib.SeerHipError):
        ops.layernorm(torch.zeros(4, 8, dtype=torch.bfloat16), torch.ones(8), torch.zeros(8))
    m = SeerUNet(block_out_channels=(32, 64, 64, 64), cross_attention_dim=64)
    with pytest.raises(_lib.SeerHipError):
        m(torch.zeros(1, 4, 2, 16, 16), 3, torch.zeros(1, 2, 77, 64))


def test_product_never_imports_oracle():
    for p in (ROOT / "seervideoldm_amd").rglob("*.py"):
        src = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{p} imports the oracle"
    assert not re.search(r"/root/reference", (ROOT / "bench.py").read_text())


def test_state_dict_surface_matches_reference_inventory():
    """SURVEY section 4 pins: 1006 keys / 1082.77 M params for the SD-v1-5-shaped SeerUNet, 223.25 M temporal."""
    from seervideoldm_amd import synth
    sh = synth.unet_param_shapes({})
    assert len(sh) == 1006
    n = lambda keys: sum(int(torch.Size(sh[k]).numel()) for k in keys if not k.endswith("freqs"))
    assert abs(n(sh) / 1e6 - 1082.77) < 0.01
    assert abs(n([k for k in sh if "temporal_attentions" in k]) / 1e6 - 223.25) < 0.01
    assert sum(k.startswith("down_blocks") for k in sh) == 366 and sum(k.startswith("mid_block") for k in sh) == 66
    assert sum(k.startswith("up_blocks") for k in sh) == 564
    assert sh["down_blocks.0.temporal_attentions.0.transformer_blocks.0.attn1.rotary_emb.freqs"] == (16,)
