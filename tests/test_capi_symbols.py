"""CPU: the C-ABI library loads without a GPU and exports every symbol include/slam_hip.h declares
(no compute calls here)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from slam_llm_amd import lib
    names = header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib.raw(), n), f"{n} declared in include/slam_hip.h but not exported by libslamhip.so"
    assert lib.raw().slam_abi_version() == lib.ABI_VERSION == 2
    assert lib.raw().slam_target_arch() == b"gfx950"


def test_binding_table_matches_header():
    from slam_llm_amd import lib
    declared = set(header_functions()) - {"slam_last_error", "slam_abi_version", "slam_target_arch"}
    assert declared == set(lib.SIGNATURES), declared ^ set(lib.SIGNATURES)
    # argument counts agree with the header prototypes
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slam_hip.h")).read(), flags=re.S)
    for name, argtypes in lib.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\((.*?)\);", src, flags=re.S)
        assert m, name
        nargs = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert nargs == len(argtypes), f"{name}: header has {nargs} args, binding has {len(argtypes)}"


def test_errors_are_reported_not_swallowed():
    """argument validation happens before any launch, so it is checkable without a GPU"""
    import ctypes
    import pytest
    from slam_llm_amd import lib
    with pytest.raises(lib.SlamHipError, match="null operand"):
        lib.call("slam_gemm_bf16_nt", None, 64, None, 64, None, 64, 8, 8, 64, None, None, 0, 0, 0, 1.0, 0, 0, None)
    one = ctypes.c_void_p(16)
    with pytest.raises(lib.SlamHipError, match="multiple of 64"):
        lib.call("slam_gemm_bf16_nt", one, 40, one, 40, one, 8, 8, 8, 40, None, None, 0, 0, 0, 1.0, 0, 0, None)
    with pytest.raises(lib.SlamHipError, match="head_dim"):
        lib.call("slam_attn_fwd", one, 64, one, 64, None, one, 64, one, 64, None, None, 1, 8, 8, 64, 64, 1, 1, 32, 0, 1.0, None, None, None, None, 0, 0, 0.0, 0, None)
    with pytest.raises(lib.SlamHipError, match="Vt must be given"):      # neither the row-major V nor its transposed copy
        lib.call("slam_attn_fwd", one, 64, one, 64, None, None, 0, one, 64, None, None, 1, 8, 8, 64, 64, 1, 1, 64, 0, 1.0, None, None, None, None, 0, 0, 0.0, 0, None)


def test_product_never_imports_the_oracle():
    """the oracle is test infrastructure: nothing under slam_llm_amd/ may import or execute it"""
    pkg = os.path.join(ROOT, "slam_llm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f"{f} imports the oracle"


# ---- which kernel a GEMM runs on: slam_gemm_kernel_name (host code only: no device is touched) ---------------------------------------
W4, PIPE, PERSIST = "gemm_nt_w4_kernel<256,256,false,0>", "gemm_nt_pipe_kernel<256,256,2,4,1>", "gemm_nt_persist2_kernel<256,256,2,4>"
T128, T128x64, TS = "gemm_nt_kernel<128,128,2,2>", "gemm_nt_kernel<128,64,2,2>", "gemm_ts_kernel"
# (forced config, M, N, K, label) for dense operands and no workspace, recorded from the Python copy of the selection rule that
# ops.gemm_kernel_name was before the library answered the question itself: the step's own products, the t256 == t128 tie (257 x 204800),
# N <= 64 on both sides of M = 4096 and of K = 256, N < 2048 against N >= 2048 at K > 2048, K = 2048 against 2112, products the 128 x 128
# tile wins, and two shapes under every forced config.  No mid-M split-K candidate (tiles256 <= 128 and N >= 256 and K >= 2048): whether
# those split depends on a registered workspace, and the GPU tests assert their labels (test_ops_gpu.py: test_gemm_mid_m_rule_*).
FROZEN_LABELS = [
    (0, 11780, 4096, 4096, W4), (0, 11780, 6144, 4160, W4), (0, 11780, 4096, 14336, W4), (0, 11780, 28672, 4096, W4),
    (0, 6000, 3840, 1280, PERSIST), (0, 6000, 5120, 1280, PERSIST), (0, 12000, 3840, 1280, PERSIST), (0, 12000, 1280, 5120, PIPE),
    (0, 12000, 5120, 1280, PERSIST), (0, 12000, 1280, 1280, PERSIST),
    (0, 4096, 128256, 4096, W4), (0, 4096, 4096, 128256, W4), (0, 128256, 4096, 4096, W4),
    (0, 257, 204800, 4096, T128), (0, 257, 204800, 1280, T128),
    (0, 672, 64, 12288, TS), (0, 4096, 64, 6144, TS), (0, 4097, 64, 6144, T128x64), (0, 11780, 64, 6144, T128x64), (0, 672, 64, 192, T128x64),
    (0, 672, 32, 256, TS), (0, 11780, 32, 4096, T128x64),
    (0, 11780, 1280, 5120, PIPE), (0, 11780, 2044, 4096, PIPE), (0, 11780, 2048, 4096, W4),
    (0, 11780, 4096, 2048, PERSIST), (0, 11780, 4096, 2112, W4),
    (0, 256, 256, 128, T128), (0, 300, 260, 64, T128), (0, 6000, 1280, 1280, T128), (0, 1000, 768, 1024, T128), (0, 4352, 4096, 1024, PERSIST),
    (0, 70, 4096, 1024, T128), (0, 129, 132, 640, T128),
    (1, 512, 512, 128, T128), (1, 1000, 768, 4096, T128),
    (2, 512, 512, 128, "gemm_nt_kernel<256,128,4,2>"), (2, 1000, 768, 4096, "gemm_nt_kernel<256,128,4,2>"),
    (3, 512, 512, 128, T128x64), (3, 1000, 768, 4096, T128x64),
    (4, 512, 512, 128, "gemm_nt_kernel<256,256,2,4>"), (4, 1000, 768, 4096, "gemm_nt_kernel<256,256,2,4>"),
    (6, 512, 512, 128, PIPE), (6, 1000, 768, 4096, PIPE),
    (7, 512, 512, 128, PERSIST), (7, 1000, 768, 4096, PERSIST),
    (11, 512, 512, 128, "gemm_nt_pipe_kernel<128,128,2,2,1>"), (11, 1000, 768, 4096, "gemm_nt_pipe_kernel<128,128,2,2,1>"),
    (12, 512, 512, 128, W4), (12, 1000, 768, 4096, W4),
]


def frozen_label_mismatches(ops):
    bad = []
    try:
        for cfg, M, N, K, want in FROZEN_LABELS:
            ops.gemm_set_config(cfg)
            got = ops.gemm_kernel_name(M, N, K)
            if got != want:
                bad.append((cfg, M, N, K, got, want))
    finally:
        ops.gemm_set_config(0)
    return bad


def test_gemm_kernel_labels_did_not_move():
    from slam_llm_amd import lib, ops
    assert len(FROZEN_LABELS) >= 40
    for cfg, M, N, K, _ in FROZEN_LABELS:
        tiles256 = ((M + 255) // 256) * ((N + 255) // 256)
        assert not (cfg == 0 and tiles256 <= 128 and N >= 256 and K >= 2048), (M, N, K)
    try:
        assert frozen_label_mismatches(ops) == []
        assert lib.raw().slam_gemm_get_config() == 0
    finally:
        ops.reset_tuning()


def test_gemm_kernel_labels_follow_the_fall_backs():
    """what the dispatch does and the Python copy of the rule did not know: the pipelined loops need two k-tiles, the descriptor kernels
    operands that 32 bits address, the tall-skinny kernel K >= 256 and an epilogue other than act 3"""
    from slam_llm_amd import ops
    try:
        ops.gemm_set_config(7)
        assert ops.gemm_kernel_name(512, 512, 64) == PIPE
        ops.gemm_set_config(11)
        assert ops.gemm_kernel_name(512, 512, 64) == T128
        ops.gemm_set_config(12)
        assert 70000 * 32768 * 2 > 2 ** 32
        assert ops.gemm_kernel_name(70000, 512, 4096, lda=32768) == PIPE
        assert ops.gemm_kernel_name(70000, 512, 4096) == W4
        ops.gemm_set_config(0)
        assert ops.gemm_kernel_name(672, 64, 12288) == TS
        assert ops.gemm_kernel_name(672, 64, 12288, act=ops.ACT_SWIGLU_BWD) == T128x64
        assert ops.gemm_kernel_name(672, 64, 192) == T128x64
    finally:
        ops.reset_tuning()


def test_reset_tuning_restores_the_library_defaults():
    from slam_llm_amd import lib, ops
    try:
        for code in (6, 106, 207, 611, 360, 370, 302, 336, 348, 401):
            ops.gemm_set_config(code)
        lib.call("slam_gemm_set_group_m", 5)
        lib.call("slam_gemm_set_group_m_rule", 3, 5, 7, 2)
        assert lib.raw().slam_gemm_get_config() == 6 and ops.gemm_kernel_name(11780, 4096, 4096) == PIPE
        ops.gemm_set_config(0)      # (the auto rule under the changed knobs: the 8-wave kernel for long K, no tall-skinny kernel)
        assert ops.gemm_kernel_name(11780, 4096, 4096) == PIPE and ops.gemm_kernel_name(672, 64, 12288) == T128x64
        ops.gemm_set_config(6)
        ops.reset_tuning()
        assert lib.raw().slam_gemm_get_config() == 0
        assert frozen_label_mismatches(ops) == []
    finally:
        ops.reset_tuning()


def test_reset_tuning_replays_the_environment_overrides():
    """a sweep's SLAM_GEMM_* environment holds at import and again after reset_tuning() (a fresh child process: the overrides are read once, at import)"""
    child = (
        "from slam_llm_amd import ops\n"
        "def labels(): return [ops.gemm_kernel_name(11780, 4096, 4096), ops.gemm_kernel_name(672, 64, 12288)]\n"
        "first = labels()\n"
        "ops.gemm_set_config(112); ops.gemm_set_config(371); ops.gemm_set_config(7)\n"
        "ops.reset_tuning()\n"
        "print(repr((first, labels())))\n")
    env = dict(os.environ, SLAM_GEMM_BIG="6", SLAM_GEMM_TS="0")
    out = subprocess.run([sys.executable, "-c", child], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == repr(([PIPE, T128x64], [PIPE, T128x64]))


# ---- which kernels an attention call runs on: slam_attn_kernel_name / slam_attn_needs_transposed (host code only: no device is touched) ----
# (slam_attn_set_fwd_qf codes, backward variant, backward, B, Tq, Tk, Hq, Hkv, D, ldq, ldk, ldv, lddo, causal, present, kernels, needs_transposed)
# present: 1 dropout, 2 relative position bias, 4 V row-major, 8 Vt copy, 16 key mask, 32 packed segments, 64 LSE output, 128 pre-scaled Q.
# Recorded from the commit BEFORE attn_plan() existed, which could not name its kernels: a scratch copy of that attention.hip whose
# attn_launch stored the kernel it was handed (resolved to its name and template arguments through the symbol table of the recording
# build) instead of launching it, with the LDS-limit and launch-error calls skipped, driven through slam_attn_fwd / slam_attn_bwd /
# slam_attn_needs_transposed by ctypes with dummy non-null pointers (nothing is dereferenced on the host); Tqp / Tkp = T rounded up to 64.
# Rows: both head sizes causal and not, the mask-free and pre-scaled-Q forms and what switches them off (key mask, segments), RP / DROP,
# V / Vt / both, K and row-major V beyond 2 GiB (the fourth row of that group: QF 2 on register-staged tiles, because the QF rule looks
# at the K-side copy and the DMA rule at the row-major V), every forward knob and the stamping variant 14; backward: Tq = 64 | 65,
# dropout / bias / GQA / key mask / segments, row-major operands beyond 2 GiB, the copies beyond 2 GiB under knob 40, variants 1 2 11 12
# 14 15 19 at D = 128 causal and variants above 10 where they take the normal path, knob 40, cross-attention.
ATTN_FROZEN = [
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 1, 68, "attn_fwd_kernel<64,true,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 4, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 132, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,true>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 196, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 84, "attn_fwd_kernel<64,false,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 1, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 36, "attn_fwd_kernel<64,false,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 68, "attn_fwd_kernel<128,true,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 0, 68, "attn_fwd_kernel<128,false,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 84, "attn_fwd_kernel<128,true,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 1, 200, 200, 4, 4, 64, 768, 768, 768, 768, 1, 100, "attn_fwd_kernel<64,true,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 70, "attn_fwd_kernel<64,false,2,true,false,false,true,false,true,false>", 2),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 69, "attn_fwd_kernel<64,false,2,false,true,false,true,false,true,false>", 2),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 71, "attn_fwd_kernel<64,false,2,true,true,false,true,false,true,false>", 2),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 72, "attn_fwd_kernel<64,false,2,false,false,false,true,true,false,false>", 0),
    ((), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 76, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 72, "attn_fwd_kernel<128,true,2,false,false,false,true,false,false,false>", 0),
    ((), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 76, "attn_fwd_kernel<128,true,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 0, 16, 32768, 32768, 8, 8, 128, 3072, 3072, 3072, 3072, 1, 68, "attn_fwd_kernel<128,true,1,false,false,false,false,false,true,false>", 2),
    ((), 0, 0, 16, 32768, 32768, 16, 16, 64, 3072, 3072, 3072, 3072, 1, 68, "attn_fwd_kernel<64,true,2,false,false,false,false,false,true,false>", 2),
    ((), 0, 0, 16, 32768, 32768, 16, 16, 64, 3072, 3072, 3072, 3072, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,false,false,true,false>", 2),
    ((), 0, 0, 4, 32768, 32768, 8, 8, 128, 1024, 1024, 8192, 1024, 1, 68, "attn_fwd_kernel<128,true,2,false,false,false,false,false,true,false>", 2),
    ((), 0, 0, 4, 32768, 32768, 8, 8, 128, 1024, 1024, 8192, 1024, 1, 76, "attn_fwd_kernel<128,true,2,false,false,false,false,false,true,false>", 2),
    ((1,), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 68, "attn_fwd_kernel<128,true,1,false,false,false,true,false,true,false>", 0),
    ((1,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,1,false,false,false,true,false,true,false>", 0),
    ((2,), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 68, "attn_fwd_kernel<128,true,2,false,false,false,true,false,true,false>", 0),
    ((2,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((10,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,false,false,true,false>", 0),
    ((10,), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 68, "attn_fwd_kernel<128,true,1,false,false,false,false,false,true,false>", 0),
    ((30,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,true,false,true,false>", 0),
    ((40,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 3),
    ((40,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 76, "attn_fwd_kernel<64,false,2,false,false,false,true,true,false,false>", 3),
    ((40,), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 72, "attn_fwd_kernel<128,true,2,false,false,false,true,false,false,false>", 3),
    ((40,), 0, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 76, "attn_fwd_kernel<128,true,2,false,false,false,true,false,false,false>", 3),
    ((60,), 0, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 132, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 14, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 0, 76, "attn_fwd_kernel<64,false,2,false,false,true,true,false,false,false>", 2),
    ((), 14, 0, 2, 200, 200, 4, 4, 64, 768, 768, 768, 768, 1, 76, "attn_fwd_kernel<64,true,2,false,false,false,true,false,true,false>", 2),
    ((), 14, 0, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1536, 1, 68, "attn_fwd_kernel<128,true,2,false,false,false,true,false,true,false>", 2),
    ((), 0, 1, 1, 64, 64, 2, 2, 64, 384, 384, 384, 128, 1, 0, "attn_bwd_dq_kernel<64,true,false,1,false> + attn_bwd_dkdv_tr_kernel<64,true>", 2),
    ((), 0, 1, 1, 65, 65, 2, 2, 64, 384, 384, 384, 128, 1, 0, "attn_bwd_dq_tr_kernel<64,true,2> + attn_bwd_dkdv_tr_kernel<64,true>", 0),
    ((), 0, 1, 1, 64, 64, 2, 2, 64, 384, 384, 384, 128, 0, 0, "attn_bwd_dq_kernel<64,false,false,1,false> + attn_bwd_dkdv_tr_kernel<64,false>", 2),
    ((), 0, 1, 1, 65, 65, 2, 2, 64, 384, 384, 384, 128, 0, 0, "attn_bwd_dq_tr_kernel<64,false,2> + attn_bwd_dkdv_tr_kernel<64,false>", 0),
    ((), 0, 1, 1, 64, 64, 2, 2, 128, 768, 768, 768, 256, 1, 0, "attn_bwd_dq_kernel<128,true,false,1,false> + attn_bwd_dkdv_tr_kernel<128,true>", 2),
    ((), 0, 1, 1, 65, 65, 2, 2, 128, 768, 768, 768, 256, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_tr_kernel<128,true>", 0),
    ((), 0, 1, 1, 64, 64, 2, 2, 128, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_kernel<128,false,false,1,false> + attn_bwd_dkdv_tr_kernel<128,false>", 2),
    ((), 0, 1, 1, 65, 65, 2, 2, 128, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_tr_kernel<128,false,2> + attn_bwd_dkdv_tr_kernel<128,false>", 0),
    ((), 0, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 1, "attn_bwd_dq_kernel<64,false,true,1,false> + attn_bwd_dkdv_kernel<64,false,true,false>", 2),
    ((), 0, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 2, "attn_bwd_dq_kernel<64,false,false,1,true> + attn_bwd_dkdv_kernel<64,false,false,true>", 2),
    ((), 0, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 3, "attn_bwd_dq_kernel<64,false,true,1,true> + attn_bwd_dkdv_kernel<64,false,true,true>", 2),
    ((), 0, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_tr_kernel<128,true>", 0),
    ((), 0, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 16, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_tr_kernel<128,true>", 0),
    ((), 0, 1, 1, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 32, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_tr_kernel<128,true>", 0),
    ((), 0, 1, 16, 32768, 32768, 8, 8, 128, 3072, 3072, 3072, 1024, 1, 0, "attn_bwd_dq_kernel<128,true,false,2,false> + attn_bwd_dkdv_kernel<128,true,false,false>", 2),
    ((), 0, 1, 16, 32768, 32768, 16, 16, 64, 3072, 3072, 3072, 1024, 0, 0, "attn_bwd_dq_kernel<64,false,false,2,false> + attn_bwd_dkdv_kernel<64,false,false,false>", 2),
    ((40,), 0, 1, 2048, 65, 65, 32, 32, 128, 4096, 4096, 4096, 4096, 1, 0, "attn_bwd_dq_kernel<128,true,false,2,false> + attn_bwd_dkdv_kernel<128,true,false,false>", 3),
    ((), 0, 1, 2048, 65, 65, 32, 32, 128, 4096, 4096, 4096, 4096, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_tr_kernel<128,true>", 0),
    ((), 1, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_kernel<128,true,false,1,false> + attn_bwd_dkdv_kernel<128,true,false,false>", 2),
    ((), 1, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_kernel<64,false,false,1,false> + attn_bwd_dkdv_kernel<64,false,false,false>", 2),
    ((), 2, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_kernel<128,true,false,2,false> + attn_bwd_dkdv_tr_kernel<128,true>", 2),
    ((), 2, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_kernel<64,false,false,2,false> + attn_bwd_dkdv_tr_kernel<64,false>", 2),
    ((), 11, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_ring_kernel<128,true,1>", 2),
    ((), 12, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_ring_kernel<128,true,2>", 2),
    ((), 14, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_ring_kernel<128,true,2,true> + attn_bwd_dkdv_ring_kernel<128,true,0>", 2),
    ((), 15, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_ring_kernel<128,true,5>", 2),
    ((), 19, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_tr_kernel<128,true,2> + attn_bwd_dkdv_ring_kernel<128,true,9>", 2),
    ((), 11, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 1, 0, "attn_bwd_dq_tr_kernel<64,true,2> + attn_bwd_dkdv_tr_kernel<64,true>", 2),
    ((), 12, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 0, 0, "attn_bwd_dq_tr_kernel<128,false,2> + attn_bwd_dkdv_tr_kernel<128,false>", 2),
    ((), 14, 1, 1, 64, 64, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_kernel<128,true,false,1,false> + attn_bwd_dkdv_ring_kernel<128,true,0>", 2),
    ((40,), 0, 1, 2, 200, 200, 8, 2, 128, 1536, 1536, 1536, 1024, 1, 0, "attn_bwd_dq_ring_kernel<128,true,2,false> + attn_bwd_dkdv_ring_kernel<128,true,0>", 3),
    ((40,), 0, 1, 2, 200, 200, 4, 4, 64, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_ring_kernel<64,false,2,false> + attn_bwd_dkdv_ring_kernel<64,false,0>", 3),
    ((40,), 0, 1, 1, 64, 64, 4, 4, 64, 768, 768, 768, 256, 0, 0, "attn_bwd_dq_kernel<64,false,false,1,false> + attn_bwd_dkdv_ring_kernel<64,false,0>", 3),
    ((), 0, 0, 2, 100, 300, 4, 4, 64, 256, 512, 512, 256, 0, 68, "attn_fwd_kernel<64,false,2,false,false,false,true,true,true,false>", 0),
    ((), 0, 0, 2, 100, 300, 8, 8, 128, 1024, 2048, 2048, 1024, 0, 84, "attn_fwd_kernel<128,false,2,false,false,false,true,false,true,false>", 0),
    ((), 0, 1, 2, 100, 300, 4, 4, 64, 256, 512, 512, 256, 0, 0, "attn_bwd_dq_tr_kernel<64,false,2> + attn_bwd_dkdv_tr_kernel<64,false>", 0),
    ((), 0, 1, 2, 100, 300, 8, 8, 128, 1024, 2048, 2048, 1024, 0, 0, "attn_bwd_dq_tr_kernel<128,false,2> + attn_bwd_dkdv_tr_kernel<128,false>", 0),
    ((), 0, 1, 2, 40, 300, 4, 4, 64, 256, 512, 512, 256, 0, 0, "attn_bwd_dq_kernel<64,false,false,1,false> + attn_bwd_dkdv_tr_kernel<64,false>", 2),
]


def attn_row_mismatches(rows, set_knobs=True):
    from slam_llm_amd import lib, ops
    bad = []
    for knobs, variant, bwd, B, Tq, Tk, Hq, Hkv, D, ldq, ldk, ldv, lddo, causal, present, want, want_needs in rows:
        if set_knobs:
            lib.call("slam_reset_tuning")
            for k in knobs:
                lib.call("slam_attn_set_fwd_qf", k)
            lib.call("slam_attn_set_bwd_variant", variant)
        got = ops.attn_kernel_name(bwd, B, Tq, Tk, Hq, Hkv, D, ldq, ldk, ldv, lddo, causal, present)
        needs = lib.raw().slam_attn_needs_transposed(B, Tq, Tk, Hq, Hkv, D, ldq, ldk, ldv, lddo, present & 3)
        # variants 0 1 2 (production, the suite, ops.attn_bwd) and the knobs: the recorded answer.  The tools' variants above 10 used to
        # ask for Qt / Kt / dOt whatever ran; the answer may narrow to what the planned kernels read, never widen
        needs_ok = needs == want_needs if variant <= 2 else (needs & 2) <= (want_needs & 2)
        if got != want or not needs_ok:
            bad.append((knobs, variant, bwd, B, Tq, Tk, D, causal, present, got, want, needs, want_needs))
    return bad


def test_attn_kernel_labels_did_not_move():
    from slam_llm_amd import ops
    assert len(ATTN_FROZEN) >= 60 and len(set(r[:15] for r in ATTN_FROZEN)) == len(ATTN_FROZEN)
    assert len(set(r[15] for r in ATTN_FROZEN)) >= 40      # (that many different launches are pinned)
    try:
        assert attn_row_mismatches(ATTN_FROZEN) == []
    finally:
        ops.reset_tuning()


def test_reset_tuning_restores_the_attention_defaults():
    from slam_llm_amd import lib, ops
    defaults = [r for r in ATTN_FROZEN if r[0] == () and r[1] == 0]
    assert len(defaults) >= 40
    try:
        for code in (1, 10, 20, 30, 40, 50, 60):
            lib.call("slam_attn_set_fwd_qf", code)
        lib.call("slam_attn_set_bwd_variant", 2)
        assert len(attn_row_mismatches(defaults, set_knobs=False)) >= 20     # (the knobs are felt)
        ops.reset_tuning()
        assert attn_row_mismatches(defaults, set_knobs=False) == []
    finally:
        ops.reset_tuning()
