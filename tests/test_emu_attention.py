"""Paged attention as an OPERATION -- the decode kernel in each product form, the context-split kernels, the prompt-pass kernels
over their work lists and the two KV-page writers -- through ntts_k_attn_decode_probe / ntts_k_attn_prefill_probe against
tests/attention_spec.py.  This module holds the case tables and the comparison helpers and runs them on the CPU SIMT emulator;
tests/test_gpu_attention.py runs the same cases on the device.

Inputs: q and k on a lattice (multiples of 1/4, |k| <= 1, |q| <= 1 or 4), so every dot product is exact in fp32 in any order and a
score cannot flip; gaussian bf16 v.  Every pool page no block table names, every slot past a context, the output buffers and the
k columns of a decode row hold bf16 NaN: whatever a guard lets through reaches the output.  Block tables are permuted, and their
unused entries name a poisoned page of the pool -- every index a kernel can form stays inside the buffers.

Tolerance (attention_spec.tolerance): |got - ref| <= ulp_bf16(ref) + 2^-12 sum_k P_k |v_k| per element -- independent of the kernel,
so the emulator and the GPU share it -- and at most 2 % of a case's outputs may differ from the spec at all (the cap of the
project's GEMM tests; an fp32 evaluation in another summation order differs in <= 0.1 %, profiles/attention_parity.txt).

Where the plain bound is not enough, and why.  The contract's softmax is fp32 (torch); the spec evaluates it in float64.  Where the float64 value of a P lies
within 2^-21 (8 fp32 ulps) of a bf16 rounding boundary, fp32 may round that P to the other neighbour -- correctly.  If the P is a large one this moves the
output by up to ulp_bf16(P) |v| = 2^-8 P |v|, which the bound's accumulation term does not cover.  Measured, emulator and MI355X alike: decode form nt2048,
group 1, the row with 63 cached tokens has a P of about 0.1 that lies 4e-8 (relative) from a boundary; the kernel takes the other neighbour, 16 of the
head's 64 outputs differ from the spec, one by 1.17 x the plain bound -- and with that one P flipped in the spec all 64 are the kernel's bit for bit.
So attention_spec.attention names such keys and returns `slack` = sum over them of ulp_bf16(P_k) |v_k| (zero in nearly every row), which `compare` adds
to the bound for those rows only; it prints how many rows hold such a P and how many outputs the slack decided (at most 25 of 5.8 million per line of
profiles/attention_parity.txt).  Everywhere else the bound is the plain one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attention_spec as sp
from neutts import _hip

PAGE = sp.PAGE
NKV = 2
SHARE_CAP = 0.02
# form id (include/neutts_hip.h ntts_k_attn_decode_form) -> (head_dim, score rows, waves)
FORMS = {"ds4": (0, 64, 2048, 8), "ds2": (1, 64, 2048, 8), "w8": (2, 64, 2048, 8), "nt1024": (3, 64, 1024, 4), "nt2048": (4, 64, 2048, 4),
         "w4_1024": (5, 64, 1024, 4), "w4_2048": (6, 64, 2048, 4), "hd128_1024": (7, 128, 1024, 4), "hd128_2048": (8, 128, 2048, 4)}
FORM_SPLIT = 9
P_ALL = [0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 255, 256, 257, 1022, 1023]      # 128 / 256: one page beyond 4 / 8 waves' first round
P_2048 = [1024, 2046, 2047]
DECODE_CASES = [(f, g) for f, (_, hd, _, _) in FORMS.items() for g in ((1, 2, 4) if hd == 128 else (1, 2, 7, 8))]
SPLIT_P = [0, 40, 159, 160, 895, 896, 1023]                                        # 5 pages over 4 chunks (159), fewer pages than chunks
SPLIT_N = [2, 3, 8, 32]
XCD_CASES = [(64, 8), (128, 4), (256, 2), (512, 1)]


def device_of(lib_path):
    return "cuda" if torch.cuda.is_available() and "emu" not in lib_path else "cpu"


def backend_of(lib_path):
    return "emu" if "emu" in lib_path else "gpu"


def _dev(a, dev):
    a = np.array(a, copy=True, order="C")                                      # (a copy: on the emulator the "device" is host memory)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def compare(label, lib_path, got_bits, ref, mag, slack):
    """got_bits uint16 [...] against the spec's bf16 values `ref` (float64): no NaN, every element inside the tolerance, and the share of
    elements that are not the spec's own bits (printed: a measurement) under the cap.  `slack` (attention_spec.attention) is zero except in the
    rows where the float64 spec cannot say which way an fp32 softmax rounds a P; their number is printed."""
    got = sp.bits_to_f32(got_bits).astype(np.float64)
    assert not np.isnan(got).any(), f"{label}: {int(np.isnan(got).sum())} NaN outputs, first at {np.argwhere(np.isnan(got))[0]}"
    err = np.abs(got - ref)
    tol = sp.tolerance(ref, mag) + slack
    bad = err > tol
    share = float((got != ref).mean())
    print(f"attention-parity {backend_of(lib_path)} {label}: {share:.5f} of {got.size} outputs differ from the spec, worst err / tol {float((err / tol).max()):.3f}, "
          f"{int((slack > 0).any(-1).sum())} of {slack.shape[0]} rows hold an ambiguous P, {int((err > tol - slack).sum())} outputs inside the tolerance by its slack alone")
    assert not bad.any(), f"{label}: {int(bad.sum())} outputs beyond the tolerance, first at {np.argwhere(bad)[0]}: got {got[bad][0]}, spec {ref[bad][0]}"
    assert share <= SHARE_CAP, f"{label}: {share:.4f} of the outputs differ from the spec"
    return share


# ================================================================================================ decode
@functools.lru_cache(maxsize=None)
def decode_case(hd, max_ctx, nw, group, qamp, plist, seed, n_stopped=1):
    """One launch: a batch row per context length in `plist` (tokens already cached; the new token sits at position P), plus a stopped row.
    The row maximum of the first head of each kv group is planted (by exchanging two keys) at key 0, the last key of page 0, the first key
    of the page the highest wave owns first, the first key of the last page, or key P -- in turn over the rows."""
    rng = np.random.default_rng(seed)
    nh = group * NKV
    P = np.array(list(plist) + [40] * n_stopped)
    B = len(P)
    state = np.array([1] * len(plist) + [0] * n_stopped, dtype=np.int32)
    max_pages = max_ctx // PAGE
    npg = P // PAGE + 1
    num_pages = int(npg.sum()) + 3
    perm = rng.permutation(num_pages)
    bt = np.full((B, max_pages), perm[-1], dtype=np.int32)                     # unused entries: a poisoned page of the pool
    kpool, vpool = sp.new_pools(num_pages, NKV, hd)
    q = sp.lattice(rng, (B, nh, hd), qamp)
    qkv = np.full((B, (nh + 2 * NKV) * hd), sp.NAN_BITS, dtype=np.uint16)      # the k columns stay poison: the kernel must not read them
    ref = np.zeros((B, nh * hd))
    mag = np.zeros((B, nh * hd))
    slack = np.zeros((B, nh * hd))
    srange = np.zeros((B, nh))
    v_new = np.zeros((B, NKV, hd), dtype=np.uint16)
    at = 0
    for b in range(B):
        L = int(P[b]) + 1
        pages = perm[at:at + npg[b]]
        at += npg[b]
        bt[b, :npg[b]] = pages
        k = sp.lattice(rng, (L, NKV, hd), 1)
        v = sp.gaussian_bf16(rng, (L, NKV, hd))
        targets = sorted({t for t in (0, PAGE - 1, PAGE * (nw - 1), PAGE * (npg[b] - 1), L - 1) if t < L})
        tgt = targets[b % len(targets)]
        for kvh in range(NKV):
            j = int(np.argmax(k[:, kvh].astype(np.float64) @ q[b, kvh * group].astype(np.float64)))
            k[[j, tgt], kvh] = k[[tgt, j], kvh]
        sp.write_tokens(kpool, vpool, pages, 0, sp.f32_to_bits(k), None)           # K of position P is in its page already
        if L > 1:
            sp.write_tokens(kpool, vpool, pages, 0, None, sp.f32_to_bits(v[:L - 1]))   # V^T of position P is the kernel's to place
        v_new[b] = sp.f32_to_bits(v[L - 1])
        qkv[b, :nh * hd] = sp.f32_to_bits(q[b]).reshape(-1)
        qkv[b, (nh + NKV) * hd:] = v_new[b].reshape(-1)
        for kvh in range(NKV):
            hs = slice(kvh * group, (kvh + 1) * group)
            o, _, m, sr, sk = sp.attention(q[b, hs], k[:, kvh], v[:, kvh], np.full(group, L), hd)
            ref[b, kvh * group * hd:(kvh + 1) * group * hd] = o.reshape(-1)
            mag[b, kvh * group * hd:(kvh + 1) * group * hd] = m.reshape(-1)
            slack[b, kvh * group * hd:(kvh + 1) * group * hd] = sk.reshape(-1)
            srange[b, hs] = sr
    vexp = vpool.copy()
    for b in range(B):
        if state[b] == 1:
            sp.write_tokens(kpool, vexp, bt[b], int(P[b]), None, v_new[b][None])
    return dict(hd=hd, nh=nh, max_ctx=max_ctx, max_pages=max_pages, num_pages=num_pages, P=P.astype(np.int32), state=state, bt=bt, kpool=kpool,
                vpool=vpool, vpool_after=vexp, qkv=qkv, ref=ref, mag=mag, slack=slack, srange=srange)


def run_decode(lib_path, case, form, fp8_inv=0.0, nsplit=0, xcd_rows=0, slabs=False):
    lib, dev = _hip.load_library(lib_path), device_of(lib_path)
    B, nh, hd = len(case["P"]), case["nh"], case["hd"]
    qkv, kpool, vpool, bt, pos, st = (_dev(case[k], dev) for k in ("qkv", "kpool", "vpool", "bt", "P", "state"))
    if fp8_inv > 0:
        out = torch.full((B, nh * hd), 0x7F, dtype=torch.uint8, device=dev)          # e4m3 NaN
    else:
        out = _dev(np.full((B, nh * hd), sp.NAN_BITS, dtype=np.uint16), dev)
    sl = torch.full((nsplit, B, nh * hd), float("nan"), dtype=torch.float32, device=dev) if slabs else None
    rc = lib.ntts_k_attn_decode_probe(_ptr(qkv), qkv.shape[1], _ptr(out), float(fp8_inv), _ptr(kpool), _ptr(vpool), case["num_pages"], _ptr(bt),
                                      case["max_pages"], _ptr(pos), _ptr(st), B, nh, NKV, hd, case["max_ctx"], form, nsplit, xcd_rows, _ptr(sl))
    assert rc == 0, rc
    return dict(out=_host(out), kpool=_host(kpool), vpool=_host(vpool), slabs=_host(sl) if slabs else None)


def check_decode(label, lib_path, case, res):
    run = case["state"] == 1
    share = compare(label, lib_path, res["out"][run], case["ref"][run], case["mag"][run], case["slack"][run])
    assert (res["out"][~run] == sp.NAN_BITS).all(), f"{label}: a stopped row's output was written"
    assert np.array_equal(res["kpool"], case["kpool"]), f"{label}: the K pool changed"
    # the V^T pool changed at slot v_slot(P % 32) of the page of P (all head_dim rows of each kv-head of each running row) and nowhere else
    diff = res["vpool"] != case["vpool_after"]
    assert not diff.any(), f"{label}: V^T pool differs from pool + appended rows at {np.argwhere(diff)[:4].tolist()}"
    return share


def decode_parity(lib_path, form, group):
    fid, hd, lmax, nw = FORMS[form]
    plist = tuple(P_ALL + (P_2048 if lmax == 2048 else []))
    qamp = 1 if group == 1 else 4
    case = decode_case(hd, lmax, nw, group, qamp, plist, 1000 * fid + group)
    if qamp == 4:
        assert case["srange"].max() >= 8                                       # the rescaling between lanes, waves and chunks carries weight
    return check_decode(f"decode {form} group {group}", lib_path, case, run_decode(lib_path, case, fid))


def decode_fp8(lib_path, form):
    """e4m3 output: the bytes are torch's cast of the probe's own bf16 rows * out_fp8_inv, clamped to +-448."""
    fid, hd, lmax, nw = FORMS[form]
    case = decode_case(hd, lmax, nw, 7, 4, tuple(P_ALL), 77)
    inv = float(np.float32(1.0 / 0.0041))
    bf = run_decode(lib_path, case, fid)["out"]
    f8 = run_decode(lib_path, case, fid, fp8_inv=inv)["out"]
    run = case["state"] == 1
    x = torch.from_numpy(sp.bits_to_f32(bf[run]).copy()) * torch.tensor(inv, dtype=torch.float32)
    want = x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = f8[run]
    same = (got == want) | (((got & 0x7F) == 0) & ((want & 0x7F) == 0))
    assert same.all(), np.argwhere(~same)[:4].tolist()
    assert (np.abs(x.numpy()) > 448).any() and (f8[~run] == 0x7F).all()          # the clamp is exercised; stopped rows untouched


def decode_xcd(lib_path, batch, xps):
    """workgroup x takes row xcd_row(x, xps): row b of the output is the attention of row b."""
    lib = _hip.load_library(lib_path)
    fid = lib.ntts_k_attn_decode_form(batch, NKV, 2048, 0, 64)
    name = [k for k, v in FORMS.items() if v[0] == fid][0]
    rng = np.random.default_rng(batch)
    case = decode_case(64, 2048, FORMS[name][3], 2, 4, tuple(int(p) for p in rng.integers(0, 64, size=batch)), batch, n_stopped=0)
    check_decode(f"decode xcd_rows {xps} batch {batch} ({name})", lib_path, case, run_decode(lib_path, case, fid, xcd_rows=xps))


def decode_split(lib_path, nsplit):
    case = decode_case(64, 1024, 4, 7, 4, tuple(SPLIT_P), 500)
    res = run_decode(lib_path, case, FORM_SPLIT, nsplit=nsplit, slabs=True)
    share = check_decode(f"decode split {nsplit}", lib_path, case, res)
    run = case["state"] == 1
    slabs = res["slabs"][:, run]
    assert not np.isnan(slabs).any(), "a chunk slab of a running row was not written"
    acc = np.zeros_like(slabs[0])
    for ch in range(nsplit):                                                   # chunk order, fp32, one rounding: the combine kernel's rows bit for bit
        acc = acc + slabs[ch]
    assert np.array_equal(sp.f32_to_bits(acc), res["out"][run])
    return share


@pytest.mark.parametrize("form,group", DECODE_CASES)
def test_decode_emu(emu_lib, form, group):
    decode_parity(emu_lib, form, group)


@pytest.mark.parametrize("form", ["w4_2048", "w8"])
def test_decode_fp8_emu(emu_lib, form):
    decode_fp8(emu_lib, form)


@pytest.mark.parametrize("batch,xps", XCD_CASES)
def test_decode_xcd_rows_emu(emu_lib, batch, xps):
    decode_xcd(emu_lib, batch, xps)


@pytest.mark.parametrize("nsplit", SPLIT_N)
def test_decode_split_emu(emu_lib, nsplit):
    decode_split(emu_lib, nsplit)


def picker_table(lib_path):
    """the batch -> form table the comments of attn_decode_launch state, at 2 kv-heads: up to 256 workgroups four per (sequence, kv-head), up to 256
    two, up to 256 one with 8 waves, then 4 waves by score rows and load policy; head_dim 128 by score rows alone."""
    lib = _hip.load_library(lib_path)
    for batch, small in [(1, "ds4"), (8, "ds4"), (32, "ds4"), (33, "ds2"), (64, "ds2"), (65, "w8"), (128, "w8"), (129, None), (256, None), (512, None)]:
        for ctx, tag in [(1024, "1024"), (2048, "2048"), (625, "1024"), (1025, "2048")]:
            for nt in (0, 1):
                want = small or ("nt" if nt else "w4_") + tag
                assert lib.ntts_k_attn_decode_form(batch, NKV, ctx, nt, 64) == FORMS[want][0], (batch, ctx, nt)
            assert lib.ntts_k_attn_decode_form(batch, NKV, ctx, 0, 128) == FORMS["hd128_" + tag][0]
    assert lib.ntts_k_attn_decode_form(16, 4, 2048, 0, 64) == FORMS["ds4"][0] and lib.ntts_k_attn_decode_form(17, 4, 2048, 0, 64) == FORMS["ds2"][0]
    assert lib.ntts_k_attn_decode_form(0, NKV, 2048, 0, 64) < 0 and lib.ntts_k_attn_decode_form(1, NKV, 2048, 0, 96) < 0


def test_decode_form_picker(emu_lib):
    picker_table(emu_lib)


def test_decode_probe_rejects_out_of_range(emu_lib):
    """the probe checks what it can before it launches: a position at max_ctx, a block-table entry outside the pool, a 1024-row form at 2048."""
    case = dict(decode_case(64, 1024, 4, 1, 1, (0, 33), 9))
    lib, dev = _hip.load_library(emu_lib), "cpu"
    def call(**kw):
        c = dict(case, **kw)
        t = [_dev(c[k], dev) for k in ("qkv", "kpool", "vpool", "bt", "P", "state")]
        out = _dev(np.zeros((3, c["nh"] * 64), dtype=np.uint16), dev)
        return lib.ntts_k_attn_decode_probe(_ptr(t[0]), t[0].shape[1], _ptr(out), 0.0, _ptr(t[1]), _ptr(t[2]), c["num_pages"], _ptr(t[3]), c["max_pages"],
                                            _ptr(t[4]), _ptr(t[5]), 3, c["nh"], NKV, 64, c["max_ctx"], c.get("form", 5), 0, 0, None)
    assert call() == 0
    assert call(P=np.array([0, 1024, 40], dtype=np.int32)) == -1
    bad = case["bt"].copy()
    bad[1, 5] = case["num_pages"]
    assert call(bt=bad) == -1
    assert call(max_ctx=2048) == -1 and call(form=7) == -1


# ================================================================================================ prompt pass
PF_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 200, 257)
PF_CAPS = [(64, 128), (0, 128), (64, 64), (0, 0)]
PF_LONG = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100)
DEFAULT_CAPS = (512, 1024)
SPREAD_N = [1, 24, 40, 70]


def _spread_lens():
    return tuple(int(x) for x in np.random.default_rng(70).integers(33, 65, size=70))


@functools.lru_cache(maxsize=None)
def prefill_inputs(lens, group, hd, qamp, seed):
    """raw lattice q | k and gaussian v rows of the prompts, quarter-turn RoPE tables, and the spec's output for EVERY position of every prompt."""
    rng = np.random.default_rng(seed)
    nh = group * NKV
    max_ctx = (max(lens) + PAGE - 1) // PAGE * PAGE
    cos, sin = sp.quarter_turn_tables(max_ctx, hd // 2, seed)
    rows, refs, mags, slacks = [], [], [], []
    srmax = 0.0
    for L in lens:
        q, k, v = sp.lattice(rng, (L, nh, hd), qamp), sp.lattice(rng, (L, NKV, hd), 1), sp.gaussian_bf16(rng, (L, NKV, hd))
        rows.append(np.concatenate([q.reshape(L, -1), k.reshape(L, -1), v.reshape(L, -1)], axis=1))
        qr, kr = sp.rope(q, cos[:L, None], sin[:L, None]), sp.rope(k, cos[:L, None], sin[:L, None])
        ref, mag, slack = np.zeros((L, nh, hd)), np.zeros((L, nh, hd)), np.zeros((L, nh, hd))
        for kvh in range(NKV):
            for h in range(kvh * group, (kvh + 1) * group):
                o, _, m, sr, sk = sp.attention(qr[:, h], kr[:, kvh], v[:, kvh], np.arange(1, L + 1), hd)
                ref[:, h], mag[:, h], slack[:, h] = o, m, sk
                srmax = max(srmax, float(sr.max()))
        refs.append(ref.reshape(L, -1))
        mags.append(mag.reshape(L, -1))
        slacks.append(slack.reshape(L, -1))
    return dict(lens=lens, nh=nh, hd=hd, max_ctx=max_ctx, cos=cos, sin=sin, rows=rows, ref=refs, mag=mags, slack=slacks, srange=srmax)


def prefill_layout(inp, seed, pos0=None, donor_pages=None, base=0):
    """pools, a permuted block table and permuted slots for the prompts of `inp`; prompt i starts at pos0[i], its leading pages named by donor_pages[i]
    (pages below `base` belong to an earlier call)."""
    rng = np.random.default_rng(seed)
    lens = inp["lens"]
    n = len(lens)
    pos0 = [0] * n if pos0 is None else pos0
    max_pages = inp["max_ctx"] // PAGE
    need = [(L + PAGE - 1) // PAGE - p0 // PAGE for L, p0 in zip(lens, pos0)]
    num_pages = base + sum(need) + 3
    perm = base + rng.permutation(num_pages - base)
    slots = rng.permutation(n + 1)[:n].astype(np.int32)
    bt = np.full((n + 1, max_pages), perm[-1], dtype=np.int32)
    at = 0
    for i in range(n):
        own = perm[at:at + need[i]]
        at += need[i]
        lead = [] if donor_pages is None else list(donor_pages[i])
        bt[slots[i], :len(lead) + need[i]] = lead + list(own)
    return dict(pos0=np.array(pos0, dtype=np.int32), slots=slots, bt=bt, num_pages=num_pages, max_pages=max_pages)


def run_prefill(lib_path, inp, lay, caps, only_last=0, pools=None, tables=None, norms=(None, None), eps=1e-6):
    lib, dev = _hip.load_library(lib_path), device_of(lib_path)
    hd, nh = inp["hd"], inp["nh"]
    lens, pos0 = np.array(inp["lens"], dtype=np.int32), lay["pos0"]
    packed = np.concatenate([r[p0:] for r, p0 in zip(inp["rows"], pos0)], axis=0)
    T = packed.shape[0]
    qkv = _dev(sp.f32_to_bits(packed), dev)
    kp, vp = pools if pools is not None else sp.new_pools(lay["num_pages"], NKV, hd)
    kpool, vpool, bt = _dev(kp, dev), _dev(vp, dev), _dev(lay["bt"], dev)
    cos, sin = tables if tables is not None else (inp["cos"], inp["sin"])
    cd, sd = _dev(sp.f32_to_bits(cos), dev), _dev(sp.f32_to_bits(sin), dev)
    nq, nk = (None if w is None else _dev(sp.f32_to_bits(w), dev) for w in norms)
    out = _dev(np.full((T, nh * hd), sp.NAN_BITS, dtype=np.uint16), dev)
    i32p = C.POINTER(C.c_int32)
    rc = lib.ntts_k_attn_prefill_probe(_ptr(qkv), qkv.shape[1], _ptr(out), 0.0, _ptr(kpool), _ptr(vpool), lay["num_pages"], _ptr(bt), lay["bt"].shape[0],
                                       lay["max_pages"], len(lens), lens.ctypes.data_as(i32p), pos0.ctypes.data_as(i32p), lay["slots"].ctypes.data_as(i32p),
                                       nh, NKV, hd, _ptr(cd), _ptr(sd), inp["max_ctx"], _ptr(nq), _ptr(nk), eps, caps[0], caps[1], only_last)
    assert rc == 0, rc
    return dict(out=_host(out), qkv=_host(qkv), kpool=_host(kpool), vpool=_host(vpool), packed=sp.f32_to_bits(packed))


def split_rows(a, inp, lay):
    """the packed rows of each prompt."""
    n = [L - p0 for L, p0 in zip(inp["lens"], lay["pos0"])]
    return np.split(a, np.cumsum(n)[:-1])


def prefill_parity(lib_path, lens, group, hd, caps, label, seed=1):
    """every query row of every head of every prompt of one packed pass."""
    inp = prefill_inputs(tuple(lens), group, hd, 4, seed)
    assert inp["srange"] >= 8 or max(lens) < 64
    lay = prefill_layout(inp, seed)
    res = run_prefill(lib_path, inp, lay, caps)
    ref, mag, slack = (np.concatenate(inp[k]) for k in ("ref", "mag", "slack"))
    return compare(f"prefill {label} group {group} hd {hd} caps {caps}", lib_path, res["out"], ref, mag, slack), res


def prefill_spread(lib_path, caps):
    """1 / 24 / 40 / 70 short prompts: the launchers spread a group's heads over 1, 2, 4 or all heads per workgroup by the size of the pass.  What a
    prompt's rows come out as does not depend on the pass it rides in."""
    lens = _spread_lens()
    outs = {}
    for n in SPREAD_N:
        inp = prefill_inputs(lens[:n], 7, 64, 4, 70)
        lay = prefill_layout(inp, 70 + n)
        res = run_prefill(lib_path, inp, lay, caps)
        compare(f"prefill spread {n} prompts caps {caps}", lib_path, res["out"], *(np.concatenate(inp[k]) for k in ("ref", "mag", "slack")))
        outs[n] = split_rows(res["out"], inp, lay)
    for n in SPREAD_N[:-1]:
        for i in range(n):
            assert np.array_equal(outs[n][i], outs[70][i]), f"prompt {i}: the {n}-prompt pass and the 70-prompt pass differ"


def prefill_shared_prefix(lib_path, caps):
    """a second call whose prompts start at pos0 = 32 / 64 / 96 on the first prompt's leading pages."""
    a = prefill_inputs((200,), 7, 64, 4, 31)
    la = prefill_layout(a, 31)
    ra = run_prefill(lib_path, a, la, caps)
    compare(f"prefill donor caps {caps}", lib_path, ra["out"], a["ref"][0], a["mag"][0], a["slack"][0])
    donor = la["bt"][la["slots"][0]]
    lens, pos0 = (97, 150, 230), (32, 64, 96)
    b = prefill_inputs(lens, 7, 64, 4, 32)
    rows, refs, mags, slacks = [], [], [], []
    for i, (L, p0) in enumerate(zip(lens, pos0)):            # the leading tokens are the donor's; the spec's rows are those of the FULL prompt
        r = b["rows"][i].copy()
        r[:p0] = a["rows"][0][:p0]
        rows.append(r)
    nh, hd, group = b["nh"], 64, 7
    cos, sin = sp.quarter_turn_tables(256, hd // 2, 31)      # (the donor's tables, continued)
    inp = dict(b, rows=rows, cos=cos, sin=sin, max_ctx=256)
    for r in rows:
        L = r.shape[0]
        q, k, v = r[:, :nh * hd].reshape(L, nh, hd), r[:, nh * hd:(nh + NKV) * hd].reshape(L, NKV, hd), r[:, (nh + NKV) * hd:].reshape(L, NKV, hd)
        qr, kr = sp.rope(q, cos[:L, None], sin[:L, None]), sp.rope(k, cos[:L, None], sin[:L, None])
        ref, mag, slack = np.zeros((L, nh, hd)), np.zeros((L, nh, hd)), np.zeros((L, nh, hd))
        for h in range(nh):
            o, _, m, _, sk = sp.attention(qr[:, h], kr[:, h // group], v[:, h // group], np.arange(1, L + 1), hd)
            ref[:, h], mag[:, h], slack[:, h] = o, m, sk
        refs.append(ref.reshape(L, -1))
        mags.append(mag.reshape(L, -1))
        slacks.append(slack.reshape(L, -1))
    lb = prefill_layout(inp, 33, pos0=list(pos0), donor_pages=[donor[:p0 // PAGE] for p0 in pos0], base=la["num_pages"])
    pools = (np.concatenate([ra["kpool"], sp.new_pools(lb["num_pages"] - ra["kpool"].shape[0], NKV, hd)[0]]),
             np.concatenate([ra["vpool"], sp.new_pools(lb["num_pages"] - ra["vpool"].shape[0], NKV, hd)[1]]))
    rb = run_prefill(lib_path, inp, lb, caps, pools=pools)
    ref, mag, slack = (np.concatenate([r[p0:] for r, p0 in zip(x, pos0)]) for x in (refs, mags, slacks))
    compare(f"prefill shared prefix caps {caps}", lib_path, rb["out"], ref, mag, slack)
    assert np.array_equal(rb["kpool"][:ra["kpool"].shape[0]], ra["kpool"]) and np.array_equal(rb["vpool"][:ra["vpool"].shape[0]], ra["vpool"])


def prefill_only_last(lib_path, lens, caps):
    """the last layer's work lists: each prompt's last row is the full run's, bit for bit (nothing is asserted about the other rows)."""
    inp = prefill_inputs(tuple(lens), 7, 64, 4, 5)
    lay = prefill_layout(inp, 5)
    full = split_rows(run_prefill(lib_path, inp, lay, caps)["out"], inp, lay)
    last = split_rows(run_prefill(lib_path, inp, lay, caps, only_last=1)["out"], inp, lay)
    compare(f"prefill only_last lens {tuple(lens)} caps {caps}", lib_path, np.stack([f[-1] for f in full]), *(np.stack([r[-1] for r in inp[k]]) for k in ("ref", "mag", "slack")))
    for i, (f, l) in enumerate(zip(full, last)):
        assert np.array_equal(f[-1], l[-1]), f"prompt {i} (length {lens[i]}): last row differs between the full and the last-block pass"


# lengths that put the last position in the first / the last block of a work item and in each tier, per caps: with caps (64, 128) the resident tier
# ends at 64, the deep one at 128; items hold 16 blocks, dealt out from both ends
ONLY_LAST = [((1, 16, 17, 63, 64, 65, 100, 127, 128, 129, 200, 257), (64, 128)), ((5, 130, 255, 256, 257, 300, 511, 512), DEFAULT_CAPS), ((33, 64, 190), (0, 0))]
ONLY_LAST_LONG = ((513, 640, 1023, 1024, 1025, 1100), DEFAULT_CAPS)


@pytest.mark.parametrize("caps", PF_CAPS)
def test_prefill_tiers_emu(emu_lib, caps):
    prefill_parity(emu_lib, PF_LENS, 7, 64, caps, "tiers")


@pytest.mark.parametrize("group", [2, 8])
def test_prefill_groups_emu(emu_lib, group):
    prefill_parity(emu_lib, PF_LENS, group, 64, (64, 128), "tiers")


@pytest.mark.parametrize("group", [1, 2, 4])
def test_prefill_hd128_emu(emu_lib, group):
    prefill_parity(emu_lib, PF_LENS, group, 128, (0, 0), "generic")


@pytest.mark.parametrize("L", PF_LONG)
def test_prefill_default_caps_emu(emu_lib, L):
    prefill_parity(emu_lib, (L,), 7, 64, DEFAULT_CAPS, f"long {L}", seed=L)


@pytest.mark.parametrize("caps", [(0, 0), DEFAULT_CAPS])
def test_prefill_head_spreading_emu(emu_lib, caps):
    prefill_spread(emu_lib, caps)


@pytest.mark.parametrize("caps", [(64, 128), (0, 0)])
def test_prefill_shared_prefix_emu(emu_lib, caps):
    prefill_shared_prefix(emu_lib, caps)


@pytest.mark.parametrize("lens,caps", ONLY_LAST + [ONLY_LAST_LONG])
def test_prefill_only_last_emu(emu_lib, lens, caps):
    prefill_only_last(emu_lib, lens, caps)


# ================================================================================================ writers
def writer_case(lib_path, hd, generic, pos0, normed=False):
    """real RoPE tables (oracle.backbone_ref.rope_cos_sin in bf16), gaussian rows: the K pages, the V^T pages and -- generic writer -- the rotated q rows
    are the spec's bit for bit, every other pool byte and row element is untouched.  normed: qk-norm weights with identity tables, within one bf16 ulp."""
    from oracle import backbone_ref as br
    rng = np.random.default_rng(hd + pos0 + 7 * generic)
    L, group = pos0 + 45, 2
    nh = group * NKV
    max_ctx = (L + PAGE - 1) // PAGE * PAGE
    cfg = br.BackboneConfig(vocab_size=64, hidden_size=nh * hd, intermediate_size=64, num_layers=1, num_heads=nh, num_kv_heads=NKV, head_dim=hd)
    if normed:
        cos, sin = np.ones((max_ctx, hd // 2), dtype=np.float32), np.zeros((max_ctx, hd // 2), dtype=np.float32)
        wq, wk = (sp.rb32(1 + 0.1 * rng.standard_normal(hd).astype(np.float32)) for _ in range(2))
    else:
        c, s = br.rope_cos_sin(cfg, torch.arange(max_ctx), torch.bfloat16)
        cos, sin = c[0, :, :hd // 2].float().numpy(), s[0, :, :hd // 2].float().numpy()
        wq = wk = None
    rows = sp.rb32(3 * sp.gaussian_bf16(rng, (L, (nh + 2 * NKV) * hd)))
    inp = dict(lens=(L,), nh=nh, hd=hd, max_ctx=max_ctx, rows=[rows])
    lay = prefill_layout(inp, 3, pos0=[pos0], donor_pages=[list(range(pos0 // PAGE))] if pos0 else None, base=pos0 // PAGE)
    kp, vp = sp.new_pools(lay["num_pages"], NKV, hd)
    if pos0:                                                                   # the prefix pages hold some earlier call's values
        pre = sp.f32_to_bits(sp.gaussian_bf16(rng, (pos0, NKV, hd)))
        sp.write_tokens(kp, vp, lay["bt"][lay["slots"][0]], 0, pre, pre)
    res = run_prefill(lib_path, inp, lay, (0, 0) if generic else (64, 128), pools=(kp.copy(), vp.copy()), tables=(cos, sin), norms=(wq, wk))
    new = rows[pos0:]
    n = L - pos0
    q, k, v = new[:, :nh * hd].reshape(n, nh, hd), new[:, nh * hd:(nh + NKV) * hd].reshape(n, NKV, hd), new[:, (nh + NKV) * hd:].reshape(n, NKV, hd)
    if normed:
        q, k = sp.head_rms_norm(q, wq, 1e-6), sp.head_rms_norm(k, wk, 1e-6)
    cq, sq = cos[pos0:L, None], sin[pos0:L, None]
    kexp, vexp = kp.copy(), vp.copy()
    sp.write_tokens(kexp, vexp, lay["bt"][lay["slots"][0]], pos0, sp.f32_to_bits(sp.rope(k, cq, sq)), sp.f32_to_bits(v))
    qexp = sp.f32_to_bits(sp.rope(q, cq, sq)).reshape(n, -1) if generic else res["packed"][:, :nh * hd]
    assert np.array_equal(res["vpool"], vexp), "V^T pages"
    assert np.array_equal(res["qkv"][:, nh * hd:], res["packed"][:, nh * hd:]), "the k | v columns of the rows changed"
    if not normed:
        assert np.array_equal(res["kpool"], kexp), "K pages"
        assert np.array_equal(res["qkv"][:, :nh * hd], qexp), "q rows"
        return
    for name, got, want in (("K pages", res["kpool"], kexp), ("q rows", res["qkv"][:, :nh * hd], qexp)):
        g, w = sp.bits_to_f32(got).astype(np.float64), sp.bits_to_f32(want).astype(np.float64)
        live = ~np.isnan(w)
        assert np.array_equal(got[~live], want[~live]), name                    # poison stays poison
        assert (np.abs(g[live] - w[live]) <= sp.bf16_ulp(w[live])).all(), name
        share = float((g[live] != w[live]).mean())
        print(f"attention-parity {backend_of(lib_path)} writer qk-norm hd {hd} {name}: {share:.5f} differ")
        assert share < 0.002, (name, share)


# (the generic writer runs at head_dim 64 only when qk-norm weights are given -- as in the engine -- so its head_dim-64 instantiation is the qk-norm case)
WRITER_CASES = [(hd, generic, pos0) for hd, generic in ((64, False), (128, True)) for pos0 in (0, 32, 96)]


@pytest.mark.parametrize("hd,generic,pos0", WRITER_CASES)
def test_writers_emu(emu_lib, hd, generic, pos0):
    writer_case(emu_lib, hd, generic, pos0)


@pytest.mark.parametrize("hd", [64, 128])
def test_writer_qk_norm_emu(emu_lib, hd):
    writer_case(emu_lib, hd, True, 32, normed=True)
