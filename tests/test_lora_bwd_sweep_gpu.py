"""slam_lora_bwd_sweep (du and every dB of a fused LoRA group from one pass over dy) against fp64 products of the same bf16 inputs, its
use in FusedLinear.backward against the separate launches, its argument checks, and the one-launch refresh of the adapter-derived operands.

Bounds (nothing fitted to what the kernel gives):
  du:  |err| <= 2^-8 |ref| + C 2^-23 sum_n |dy b|          one final bf16 rounding + worst case of fp32 accumulation of C terms in any order
  dB:  |err| <= M 2^-23 s sum_m |dy u| + 2^-23 |old|       fp32 accumulation of M terms in any order (+ the add onto the old gradient)
"""
import ctypes

import pytest
import torch

EPS32, EPSBF = 2.0 ** -23, 2.0 ** -8

# name -> (parts, [(part index, r)], alpha)
GROUPS = {
    "qkv_r8_r16": ([128, 64, 64], [(0, 8), (2, 16)], 32.0),     # adapter-free part in the middle, sum_r 24 of Rp 64
    "gate_up_r16": ([192, 192], [(0, 16), (1, 16)], 16.0),
    "one_r32": ([128], [(0, 32)], 32.0),
    "qv_r32": ([128, 64, 64], [(0, 32), (2, 32)], 64.0),         # sum_r 64 = Rp: no padding columns
}


def _adapters(parts, spec, alpha):
    row0 = [sum(parts[:i]) for i in range(len(parts))]
    out, j0 = [], 0
    for pi, r in spec:
        out.append(dict(row0=row0[pi], rows=parts[pi], j0=j0, r=r, scale=alpha / r))
        j0 += r
    return out


_CASES = {}


def _case(name, M):
    """inputs (CPU, bf16-exact values held in fp64) and the fp64 references of one group x M: computed once, shared, never modified"""
    key = (name, M)
    if key in _CASES:
        return _CASES[key]
    parts, spec, alpha = GROUPS[name]
    ads = _adapters(parts, spec, alpha)
    N, sum_r = sum(parts), sum(a["r"] for a in ads)
    Rp = 64
    g = torch.Generator().manual_seed(1000 * M + len(name))
    bf = lambda t: t.to(torch.bfloat16)
    dy = bf(torch.randn(M, N, generator=g))
    u = bf(torch.randn(M, sum_r, generator=g))
    bt = torch.zeros(Rp, N, dtype=torch.bfloat16)
    for a in ads:
        bt[a["j0"]: a["j0"] + a["r"], a["row0"]: a["row0"] + a["rows"]] = bf(a["scale"] * 0.1 * torch.randn(a["r"], a["rows"], generator=g))
    old = [torch.randn(a["rows"], a["r"], generator=g) for a in ads]
    dy64, u64, bt64 = dy.double(), u.double(), bt.double()
    du_ref = dy64 @ bt64.T
    du_abs = dy64.abs() @ bt64.abs().T
    du_tol = EPSBF * du_ref.abs()
    for a in ads:
        sl = slice(a["j0"], a["j0"] + a["r"])
        du_tol[:, sl] += a["rows"] * EPS32 * du_abs[:, sl]
    db_ref, db_abs = [], []
    for a in ads:
        d = dy64[:, a["row0"]: a["row0"] + a["rows"]]
        uu = u64[:, a["j0"]: a["j0"] + a["r"]]
        db_ref.append(a["scale"] * (d.T @ uu))
        db_abs.append(a["scale"] * (d.abs().T @ uu.abs()))
    c = dict(ads=ads, N=N, sum_r=sum_r, Rp=Rp, dy=dy, u=u, bt=bt, old=old, du_ref=du_ref, du_tol=du_tol, db_ref=db_ref, db_abs=db_abs)
    _CASES[key] = c
    return c


def _run(dev, c, M, splits, accumulate):
    """one sweep on operands laid out like FusedLinear.backward's: dy a column view (ld > N), u / du column blocks, du with 8 spare rows"""
    from slam_llm_amd import ops
    N, Rp, sum_r = c["N"], c["Rp"], c["sum_r"]
    dyb = torch.zeros((M, N + 64), dtype=torch.bfloat16, device=dev)
    dyb[:, 32: 32 + N] = c["dy"].to(dev)
    ub = torch.zeros((M, 40 + Rp), dtype=torch.bfloat16, device=dev)
    ub[:, 40: 40 + sum_r] = c["u"].to(dev)
    dub = torch.full((M + 8, 16 + Rp), float("nan"), dtype=torch.bfloat16, device=dev)
    grads = [(o.clone() if accumulate else torch.full_like(o, float("nan"))).to(dev) for o in c["old"]]
    tab = ops.lora_adapter_table(c["ads"], grads)
    ops.lora_bwd_sweep(dyb[:, 32: 32 + N], c["bt"].to(dev), ub[:, 40:], dub[:M, 16:], tab, accumulate=accumulate, splits=splits)
    torch.cuda.synchronize()
    return dub.cpu(), [g_.cpu() for g_ in grads]


def test_reference_sits_inside_its_own_bounds():
    """CPU side of the bounds: with random-normal inputs the tolerances are a small fraction of the values they guard (a result of zeros,
    or one with a term dropped, cannot pass), and the fp64 reference rounded the way the kernel rounds (bf16 for du, fp32 for dB) passes"""
    for name in GROUPS:
        for M in (1, 31, 70, 1029):
            c = _case(name, M)
            live = c["du_ref"][:, : c["sum_r"]]
            assert (c["du_tol"][:, : c["sum_r"]] < live.abs()).double().mean() > 0.9
            assert ((live.to(torch.bfloat16).double() - live).abs() <= c["du_tol"][:, : c["sum_r"]]).all()
            for a, ref, ab, old in zip(c["ads"], c["db_ref"], c["db_abs"], c["old"]):
                tol = M * EPS32 * ab + EPS32 * old.abs().double()
                assert (tol < 0.05 * ref.abs().mean()).all()
                assert ((ref.float().double() - ref).abs() <= tol).all()
                assert (((ref.float() + old).double() - (ref + old.double())).abs() <= tol).all()


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("M", [1, 31, 70, 1029])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_sweep_matches_fp64(dev, name, M, splits):
    c = _case(name, M)
    Rp, sum_r = c["Rp"], c["sum_r"]
    for accumulate in (False, True):
        dub, grads = _run(dev, c, M, splits, accumulate)
        assert torch.isnan(dub[M:]).all() and torch.isnan(dub[:, :16]).all(), "rows >= M / columns in front of du were written"
        du = dub[:M, 16:].double()
        assert not torch.isnan(du).any()
        assert (du[:, sum_r:] == 0).all(), "padding columns [sum_r, Rp) must be exactly zero"
        err = (du - c["du_ref"]).abs()
        print(f"{name} M={M} splits={splits}: du worst err/tol {float((err / c['du_tol'].clamp_min(1e-300))[:, :sum_r].max()):.3f}")
        assert (err <= c["du_tol"]).all()
        for a, got, ref, ab, old in zip(c["ads"], grads, c["db_ref"], c["db_abs"], c["old"]):
            assert not torch.isnan(got).any()
            want = ref + old.double() if accumulate else ref
            tol = M * EPS32 * ab + (EPS32 * old.abs().double() if accumulate else 0.0)
            e = (got.double() - want).abs()
            print(f"   dB rows {a['rows']} r {a['r']} acc={accumulate}: worst err/tol {float((e / tol.clamp_min(1e-300)).max()):.3f}")
            assert (e <= tol).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,M,splits", [("qkv_r8_r16", 1029, 0), ("qv_r32", 1029, 3), ("gate_up_r16", 70, 3)])
def test_sweep_repeats_bit_equal(dev, name, M, splits):
    c = _case(name, M)
    a, ga = _run(dev, c, M, splits, True)
    b, gb = _run(dev, c, M, splits, True)
    assert torch.equal(a[:M, 16:], b[:M, 16:])
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_fused_linear_backward_sweep_vs_separate_launches(dev, monkeypatch):
    """FusedLinear.backward with the sweep against the extension product + per-adapter grams (SLAM_LORA_BWD_SWEEP=0), lora_dropout 0.05.
    Both routes compute du and dB from the same bf16 operands with fp32 accumulation, so each sits within the du / dB bound E of the
    exact value and they differ by at most 2 E.  Through the rest of the backward, with d = 2 E_du the du difference, k = 1 / (1 - p):
      dx:  the hop (du . A) is accumulated in fp32 (Rp terms), rounded to bf16, masked, scaled by k and added into the bf16 dx, rounded again:
           |ddx| <= k (d |A| + 2 Rp 2^-23 |du||A| + 2 2^-8 |du||A|) + 2 2^-8 |dx|       (|du| taken as |du_ref| + E_du)
      dA:  du^T dropout(x) over M rows in fp32:  |ddA| <= k (d^T |x| + 2 M 2^-23 |du|^T |x|)
      dB:  |ddB| <= 2 (M 2^-23 s |dy|^T |u|)"""
    from slam_llm_amd import model as MD
    from slam_llm_amd import ops
    M, K, alpha, p = 300, 128, 32.0, 0.05
    parts, spec, _ = GROUPS["qkv_r8_r16"]
    names = ["q_proj", "k_proj", "v_proj"]
    store = MD.TrainableStore(dev)
    fl = MD.FusedLinear(K, list(zip(names, parts)), dev)
    for pi, r in spec:
        store.reserve(f"{names[pi]}.A", (r, K))
    for pi, r in spec:
        store.reserve(f"{names[pi]}.B", (parts[pi], r))
        fl.add_lora(names[pi], r, alpha, f"{names[pi]}.A", f"{names[pi]}.B")
    store.allocate()
    g = torch.Generator().manual_seed(5)
    for n, rows in fl.parts:
        fl.set_base(n, (torch.randn(rows, K, generator=g) * K ** -0.5).to(dev).to(torch.bfloat16))
    fl.finalize()
    with torch.no_grad():
        for prm in store.params.values():
            prm.copy_((torch.randn(prm.shape, generator=g) * 0.1).to(dev))
    store.refresh_bf16()
    fl.refresh(store)
    x_ext = fl.new_input(M)
    x_ext[:, :K] = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    drop = (p, 77, 5 << 40)
    fl.forward(x_ext, store, drop=drop)
    dy = torch.randn(M, fl.N, generator=g).to(torch.bfloat16).to(dev)

    def run(flag):
        monkeypatch.setattr(MD, "LORA_BWD_SWEEP", flag)
        monkeypatch.setattr(MD, "LORA_BWD_SWEEP_MIN_M", 1)
        store.grad.zero_()
        dx = fl.backward(dy, x_ext, store, accumulate=False, drop=drop)
        torch.cuda.synchronize()
        return dx.double().cpu(), {n: store.grad_view(n).double().cpu().clone() for n in store.params}

    dx1, g1 = run(True)
    dx0, g0 = run(False)
    k = 1.0 / (1.0 - p)
    dy64, bt64 = dy.double().cpu(), fl.WextT[K:].double().cpu()
    u64, x64 = x_ext[:, K:].double().cpu(), x_ext[:, :K].double().cpu()
    sr, Rp = fl.sum_r, fl.Rp
    du_ref, du_abs = dy64 @ bt64.T, dy64.abs() @ bt64.abs().T
    e_du = EPSBF * du_ref.abs()
    for a in fl.adapters:
        sl = slice(a["j0"], a["j0"] + a["r"])
        e_du[:, sl] += a["rows"] * EPS32 * du_abs[:, sl]
    assert ((dx1[:, K:] - dx0[:, K:]).abs() <= 2 * e_du).all()
    d, du_mag = 2 * e_du[:, :sr], du_ref.abs()[:, :sr] + e_du[:, :sr]
    A = fl.a_cat(store).double().cpu().abs()          # [sum_r, K]
    hop = du_mag @ A
    tol_dx = k * (d @ A + 2 * Rp * EPS32 * hop + 2 * EPSBF * hop) + 2 * EPSBF * torch.maximum(dx0[:, :K].abs(), dx1[:, :K].abs())
    err = (dx1[:, :K] - dx0[:, :K]).abs()
    print(f"dx worst err/tol {float((err / tol_dx.clamp_min(1e-300)).max()):.3f}")
    assert (err <= tol_dx).all()
    tol_dA = k * (d.T @ x64.abs() + 2 * M * EPS32 * (du_mag.T @ x64.abs()))
    for a in fl.adapters:
        sl = slice(a["j0"], a["j0"] + a["r"])
        e = (g1[a["A"]] - g0[a["A"]]).abs()
        print(f"dA {a['part']} worst err/tol {float((e / tol_dA[sl].clamp_min(1e-300)).max()):.3f}")
        assert (e <= tol_dA[sl]).all()
        tol_dB = 2 * M * EPS32 * a["scale"] * (dy64[:, a["row0"]: a["row0"] + a["rows"]].abs().T @ u64[:, sl].abs())
        e = (g1[a["B"]] - g0[a["B"]]).abs()
        print(f"dB {a['part']} worst err/tol {float((e / tol_dB.clamp_min(1e-300)).max()):.3f}")
        assert (e <= tol_dB).all()
        assert g1[a["B"]].abs().max() > 0 and g1[a["A"]].abs().max() > 0


def test_sweep_rejects_bad_arguments():
    """argument validation happens before any launch (no GPU needed), with a message, like the neighbouring ops"""
    from slam_llm_amd import lib
    one = ctypes.c_void_p(16)

    def table(row0=0, rows=128, r=8, dB=16):
        t = (lib.LoraAdapter * 1)()
        t[0].row0, t[0].rows, t[0].j0, t[0].r, t[0].scale, t[0].dB = row0, rows, 0, r, 4.0, dB
        return t

    def call(tab, sum_r=8, Rp=64, dy=one, ws=one):
        lib.call("slam_lora_bwd_sweep", dy, 256, one, 256, one, 64, one, 64, 100, 256, sum_r, Rp, tab, 1, 0, 0, ws, 1 << 30, None)

    with pytest.raises(lib.SlamHipError, match="multiples of 64"):
        call(table(row0=32))
    with pytest.raises(lib.SlamHipError, match="multiples of 64"):
        call(table(rows=96))
    with pytest.raises(lib.SlamHipError, match="multiple of 8"):
        call(table(r=12), sum_r=12)
    with pytest.raises(lib.SlamHipError, match="Rp=128"):
        call(table(), Rp=128)
    with pytest.raises(lib.SlamHipError, match="null pointer"):
        call(table(), dy=None)
    with pytest.raises(lib.SlamHipError, match="null pointer"):
        call(table(dB=None))
    with pytest.raises(lib.SlamHipError, match="workspace too small"):
        lib.call("slam_lora_bwd_sweep", one, 256, one, 256, one, 64, one, 64, 100, 256, 8, 64, table(), 1, 0, 0, one, 64, None)
    assert lib.call("slam_lora_bwd_sweep_workspace_bytes", 100, 256, 8, table(row0=32), 1, 0) == -1
    assert "multiples of 64" in lib.last_error()
    assert lib.call("slam_lora_bwd_sweep_workspace_bytes", 100, 256, 8, table(), 1, 0) > 0


@pytest.mark.gpu
def test_batched_refresh_matches_per_group_refresh(dev):
    """after a real optimizer step on a 2-layer model: the one-launch refresh of LlamaHip writes every Wext[:, K:], WextT[K:] and AcatT
    bit-equal to FusedLinear.refresh group by group (the adapters' blocks are poisoned before each, so both must write all of them)"""
    from oracle import slam_oracle as O
    from slam_llm_amd.model import SlamAdamW, SlamHipModel
    cfg = O.make_config()
    model = SlamHipModel(dict(cfg, lora_dropout=0.0), dev).load_weights(O.init_weights(cfg, seed=42))
    model.train()
    ob = O.synth_batch(cfg, O.synth_audio(2, 2.0, seed=1234), prompt_len=6, answer_lens=(5, 9), seed=1236, left_pad=True, pad_to_30s=False)
    opt = SlamAdamW(model, lr=1e-2)
    for _ in range(2):          # lora_B starts at zero: after two steps both A and B have moved
        outputs, _ = model(**{k: v.to(dev) for k, v in ob.items()})
        outputs.loss.backward()
        opt.step()
        opt.zero_grad()
    llm, store = model.llm, model.llm.store
    groups = [fl for L in llm.layers for fl in (L.qkv, L.o, L.gu, L.down) if fl.adapters]
    assert len(groups) >= 2 and len(llm.layers) == 2

    def poison():
        for fl in groups:
            for a in fl.adapters:
                fl.Wext[a["row0"]: a["row0"] + a["rows"], fl.K + a["j0"]: fl.K + a["j0"] + a["r"]] = 7.0
                fl.WextT[fl.K + a["j0"]: fl.K + a["j0"] + a["r"], a["row0"]: a["row0"] + a["rows"]] = 7.0
            fl.AcatT.fill_(7.0)

    def snapshot():
        torch.cuda.synchronize()
        return [(fl.Wext[:, fl.K:].clone(), fl.WextT[fl.K:].clone(), fl.AcatT.clone()) for fl in groups]

    poison()
    llm.refresh()
    got = snapshot()
    ptrs = [fl.AcatT.data_ptr() for fl in groups]
    poison()
    for fl in groups:
        fl.refresh(store)
    want = snapshot()
    assert ptrs == [fl.AcatT.data_ptr() for fl in groups], "destinations must be refreshed in place"
    for fl, g_, w_ in zip(groups, got, want):
        for a_, b_, what in zip(g_, w_, ("Wext[:, K:]", "WextT[K:]", "AcatT")):
            assert torch.equal(a_, b_), what
        assert float(w_[0].abs().max()) > 0 and not (w_[0] == 7.0).any() and not (w_[2] == 7.0).any()
        assert float(w_[1].float().abs().max()) > 0
