"""tests/_gemm_ref.py checked without a GPU: the checker against a stand-in kernel (torch's CPU fp32 matmul over
the reference's own storage tensors), against stand-ins that are wrong on purpose, the plan mirror against the
library's host-only queries, and the argument refusals of gemm_impl that precede every launch.
test_gpu_gemm.py then holds the kernels to the same reference, bounds and table.

A check that a wrong kernel meets checks nothing: each mutation below must fail the check on every case it
applies to ("applies" is spelled out in ``applies``), and every mutation applies to at least one case.
"""
import ctypes

import pytest
import torch

from ctr_recommendation_amd import _lib
from tests import _gemm_ref as gr

CASES = gr.CASES
IDS = [c.id for c in CASES]
MUTATIONS = ("drop_k", "remap", "beta2", "bias_next", "omit_chunk", "kseg64", "lo_ignored", "truncate")


def applies(mut: str, c: gr.Case, kind: str) -> bool:
    """whether the case has the feature the mutation breaks"""
    if mut == "drop_k":
        return True
    if mut == "remap":                  # a remap to shift
        return c.rB != gr.NO_REMAP or c.rC != gr.NO_REMAP
    if mut == "beta2":
        return c.beta != 0.0
    if mut == "bias_next":
        return c.bias
    if mut == "omit_chunk":             # a K split to lose a chunk of
        return gr.resolve(c)["split"] > 1
    if mut == "kseg64":
        return c.kseg > 0
    if mut == "lo_ignored":             # integer inputs have no lo part
        return kind == "real" and (c.types == "x3" or c.entry == "s3")
    if mut == "truncate":               # an fp32 operand the kernel rounds to bf16
        return kind == "real" and c.bf16 == 1 and not (c.a16 and c.b16)
    raise KeyError(mut)


def _shift(rm):                         # 4 to the left: stays inside the storage
    return (rm[0], rm[1] - 4, rm[2] - 4)


def _trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32) if x.dtype == torch.float32 else x.float()


def standin(c: gr.Case, inp: gr.Inputs, mut=None) -> torch.Tensor:
    """the C storage a float32 kernel would leave (slab mode: the float64 sum of its slabs), optionally wrong"""
    rB = _shift(c.rB) if (mut == "remap" and c.rB != gr.NO_REMAP) else c.rB
    rC = _shift(c.rC) if (mut == "remap" and c.rB == gr.NO_REMAP) else c.rC
    kchunk = gr.resolve(c)["kchunk"]
    if c.entry == "s3":
        # one GEMM over 3 K0: [A_hi | A_hi | A_lo] x [B_hi ; B_lo ; B_hi]
        ah, al = gr.logical_a(c, inp.A[0]).float(), gr.logical_a(c, inp.A[1]).float()
        bh, bl = gr.logical_b(c, inp.B[0]).float(), gr.logical_b(c, inp.B[1]).float()
        if mut == "lo_ignored":
            al, bl = torch.zeros_like(al), torch.zeros_like(bl)
        if mut == "drop_k":
            ah, al = ah.clone(), al.clone()
            ah[:, -1] = 0
            al[:, -1] = 0
        a, b = torch.cat([ah, ah, al], 1), torch.cat([bh, bl, bh], 0)
    else:
        a = gr.logical_a(c, inp.A, inp.A2, c.kseg - 64 if mut == "kseg64" else None)
        b = gr.logical_b(c, inp.B, inp.B2, rB)
        if c.bf16 == 1:
            a, b = (_trunc(a), _trunc(b)) if mut == "truncate" else (a.bfloat16().float(), b.bfloat16().float())
        elif mut == "lo_ignored":
            a, b = a.bfloat16().float(), b.bfloat16().float()
        a, b = a.float().clone(), b.float()
        if mut == "drop_k":
            a[:, -1] = 0
    if mut == "omit_chunk":
        a = a.clone()
        a[:, :kchunk] = 0               # chunk 0: with integer inputs the later chunks of an s3 GEMM hold zeros
    out = a @ b                         # float32
    if inp.bias is not None:
        out = out + (inp.bias.roll(-1) if mut == "bias_next" else inp.bias)
    if c.beta != 0.0:
        c0 = gr.logical_c(c, inp.C0)
        out = out + c.beta * c0
        if mut == "beta2":
            out = out + c.beta * c0
    if c.entry == "slabs":
        return out.double()
    C = inp.C0.clone()
    C[:c.M, gr.remap_index(rC, c.N)] = out.to(C.dtype)
    return C


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_checker_passes_standin_and_fails_mutations(c):
    for kind in ("int", "real") if c.real_ok else ("int",):
        inp = gr.make_inputs(c, kind)
        A = (inp.A, inp.A2) if c.kseg else inp.A
        B = (inp.B, inp.B2) if c.nseg else inp.B
        C_ref, S = gr.reference(c, A, B, inp.bias, inp.C0)
        ok, ratio, msg = gr.check(c, kind, standin(c, inp), inp.C0, C_ref, S)
        assert ok, (kind, msg)
        if kind == "real":
            assert ratio < 1.0
        for mut in MUTATIONS:
            if applies(mut, c, kind):
                bad, _, _ = gr.check(c, kind, standin(c, inp, mut), inp.C0, C_ref, S)
                assert not bad, f"{kind}: the check passes a kernel with mutation {mut}"
        if c.entry == "s3" and kind == "real" and inp.A.shape == inp.B.shape:
            # the reference with the two lo images swapped is a different matrix: the honest result misses it
            R2, S2 = gr.reference(c, A, B, inp.bias, inp.C0, swap_lo=True)
            assert not gr.check(c, kind, standin(c, inp), inp.C0, R2, S2)[0]


def test_every_mutation_applies_somewhere():
    for mut in MUTATIONS:
        n = sum(applies(mut, c, kind) for c in CASES for kind in (("int", "real") if c.real_ok else ("int",)))
        assert n > 0, mut


def test_reference_is_the_documented_formula():
    """reference() on a small remapped, strided, beta / bias case against the formula of gemm.hip's header
    written out with Python loops over the storage."""
    c = gr.Case("loop", "gemm", 5, 12, 12, True, True, "f32", "", rB=(4, 4, 8), rC=(8, 0, 4), beta=2.0, bias=True)
    inp = gr.make_inputs(c, "real")
    ref, S = gr.reference(c, inp.A, inp.B, inp.bias, inp.C0)
    rm = lambda r, i: i + (r[1] if i < r[0] else r[2])
    for m in range(c.M):
        for n in range(c.N):
            acc = float(inp.bias[n]) + c.beta * float(inp.C0[m, rm(c.rC, n)])
            sab = abs(float(inp.bias[n])) + c.beta * abs(float(inp.C0[m, rm(c.rC, n)]))
            for k in range(c.K):
                t = float(inp.A[k, m]) * float(inp.B[n, rm(c.rB, k)])      # "T" A[k*lda+m], "T" B[n*ldb+rB(k)]
                acc, sab = acc + t, sab + abs(t)
            assert abs(acc - float(ref[m, n])) <= 1e-12 * sab and abs(sab - float(S[m, n])) <= 1e-12 * sab
    # rB sends k < 4 to columns 4..7 and the rest to 12..19: columns 0..3 and 8..11 are skipped; A's gap is past M
    assert bool(torch.isnan(inp.B[:, 0:4]).all()) and bool(torch.isnan(inp.B[:, 8:12]).all())
    assert bool(torch.isnan(inp.A[:, c.M:]).all())


# --------------------------------------------------------------------------------- the plan mirror
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_reaches_its_path(c):
    assert gr.resolve(c)["path"] == c.path


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mirror_matches_library_queries(c):
    h = _lib.lib()
    M, N, K = c.M, c.N, c.kk
    s = gr.plan_gemm(M, N, K, 32)["split"]
    assert h.fbn_gemm_workspace_size(M, N, K, 0) == (s * M * N * 4 if s > 1 else 0)
    for bf16 in (1, 2):
        assert h.fbn_gemm_workspace_size(M, N, K, bf16) == gr.workspace_size(M, N, K, bf16)
    assert h.fbn_gemm_slabs_split(M, N, K) == gr.slab_split(M, N, K)
    assert h.fbn_gemm_slabs_size(M, N, K) == gr.slab_split(M, N, K) * M * N * 4
    p = gr.resolve(c)
    if p["kernel"] == "dma" and not (c.entry == "bf16out"):
        assert p["split"] == gr.slab_split(M, N, K)          # the DMA split after gemm_impl's rounding


def test_table_names_every_dispatch_branch():
    paths = {c.path for c in CASES}
    gen = {c for c in CASES if c.path.startswith("generic")}
    # launch_types: fp32, split-bf16 x3 and the four bf16-compute operand variants, in every layout
    assert {(c.types, c.tA, c.tB) for c in gen} >= {(t, a, b) for t in ("f32", "bf1", "x3", "a16", "b16", "ab16")
                                                    for a, b in gr.LAYOUTS}
    # launch_sel / launch_split: the four tiles, fp32 in each, a second type in each
    for tile in ("128x128", "128x64", "64x128", "64x64"):
        ts = {c.types for c in gen if f":{tile}:" in c.path}
        assert "f32" in ts and len(ts) >= 2, tile
    assert any(c.types == "x3" and ":128x128:" in c.path for c in gen)       # launch_split beyond 64x64
    # launch_dma16_sel: 8 waves on 128x128 and 64x128, 4 waves on 64x64; rings of 2 and 4; S3; bf16 C
    for frag in ("dma:128x128:w8:ring2", "dma:64x128:w8:ring2", "dma:64x64:w4:ring2", "dma:128x128:w8:ring4",
                 "dma:64x64:w4:ring4"):
        assert any(p.startswith(frag) for p in paths), frag
        assert {(c.tA, c.tB) for c in CASES if c.path.startswith(frag)} == set(gr.LAYOUTS), frag
    # the reduce kernels, per family where both reach them
    for red in ("reduce", "reduce4", "reduce4_wide", "reduce_stats"):
        assert any(c.path == f"generic:64x64:split{s}:{red}" for c in gen for s in (2, 4, 8, 16, 32)), red
    assert any(c.path.startswith("dma") and c.path.endswith(":reduce4") for c in CASES)
    assert any(c.path.endswith(":slabs") and c.kseg for c in CASES) and any(c.path.endswith(":slabs") and c.nseg
                                                                            for c in CASES)
    assert any(c.stats and c.path.startswith("generic") and c.path.endswith(":none") for c in CASES)
    assert any(c.stats and c.path.startswith("dma:128x128:w8") for c in CASES)
    assert {c.entry for c in CASES} == {"gemm", "split", "bf16out", "s3", "slabs"}


def test_table_shapes_have_the_edges_they_claim():
    by = {c.id: c for c in CASES}
    r = gr.resolve
    assert r(by["gsplit-f32-NT"])["kchunk"] == 256 and 1000 - 3 * 256 == 232          # a K tail inside a split
    assert r(by["gsplit-bf1-NT"])["kchunk"] == 512
    p = r(by["a2-100x512x1920-NT"])
    assert (p["kchunk"], p["split"]) == (256, 8) and 2 * 256 < 640 < 3 * 256         # chunk 2 straddles kseg
    p = r(by["a2-72x64x384-NT"])
    assert (p["kchunk"], p["split"]) == (192, 2) and 0 < 128 < 192                   # chunk 0 straddles
    assert r(by["a2-64x64x256-NT"])["kchunk"] == 128                                 # none does
    for k in (1, 2, 3):                                                              # fewer K steps than stages
        c = by[f"dtiny{k}-NT"]
        assert c.K // 64 == k < 4 and r(c)["stages"] == 4 and r(c)["split"] == 1
    assert r(by["s3-200x136x128-b0-NT"])["kchunk"] == 192                            # a chunk across two K-segments
    c = by["gdv16-ab16-NT"]
    assert (c.LDA, c.LDB, c.LDC, c.beta) == (16, 16, 16, 1.0) and not gr.dma16_eligible(c)
    assert by["grbk-f32-NT"].LDB == 336 == by["grbn-f32-NN"].LDB and by["grbk-f32-NT"].rB == (80, 16, 96)
    for c in CASES:                      # every gap is real, every alignment rule of gemm_impl is met
        assert c.LDA % 4 == 0 and c.LDB % 4 == 0 and (not c.a16 or c.LDA % 8 == 0) and (not c.b16 or c.LDB % 8 == 0)
        assert c.LDA >= c.a_cols and c.LDB >= c.b_cols and c.LDC >= gr.remap_extent(c.rC, c.N)
        if c.id.split("-")[0] not in ("gdv16", "gscalar", "grbk", "grbn") and c.entry != "slabs":
            assert c.LDA > c.a_cols and c.LDB > c.b_cols and c.LDC > c.N, c.id
        assert 9 * c.K + 9 < 2 ** 24


# ------------------------------------------------------------------------------------ host refusals
PTR = 1 << 20            # a dummy 16-byte-aligned, non-null address: never dereferenced by a refused call
NR = gr.NO_REMAP


def _gemm(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, tA=0, tB=1, rB=NR, bf16=0, a16=0, b16=0):
    _lib.call("fbn_gemm", PTR, PTR, PTR, None, M, N, K, lda, ldb, ldc, tA, tB, rB[0], rB[1], rB[2], NR[0], NR[1],
              NR[2], 0.0, bf16, a16, b16, None, None, 0, None)


def _split(tA=0, tB=1, A2=None, kseg=gr.INT_MAX, lda2=0):
    _lib.call("fbn_gemm_split", PTR, PTR, PTR, None, 64, 64, 256, 256, 256, 64, tA, tB, NR[0], NR[1], NR[2], 0.0, None,
              None, 0, A2, lda2, kseg, None, 0, gr.INT_MAX, None)


REFUSALS = [
    ("lda % 4", lambda: _gemm(lda=66), "ld % 4"),
    ("bf16 A with lda % 8", lambda: _gemm(lda=68, bf16=1, a16=1), "ld % 8"),
    ("bf16 B with ldb % 8", lambda: _gemm(ldb=68, bf16=1, b16=1), "ld % 8"),
    ("bf16 B with a B remap", lambda: _gemm(ldb=128, bf16=1, b16=1, rB=(16, 8, 16)), "no B remap"),
    ("bf16 = 2 with a bf16 operand", lambda: _gemm(bf16=2, a16=1), "fp32 operands only"),
    ("A2 with transA", lambda: _split(tA=1, A2=PTR, kseg=128, lda2=128), "k-contiguous A"),
    ("kseg % 128", lambda: _split(A2=PTR, kseg=64, lda2=192), "segments % 128"),
    ("s3 with K0 % 64", lambda: _lib.call("fbn_gemm_s3", PTR, PTR, PTR, 64, 64, 32, 32, 32, 64, 0, 1, 4096, 4096, 0.0,
                                          None, 0, None), "K0 % 64"),
    ("slabs with a short workspace", lambda: _lib.call(
        "fbn_gemm_slabs", PTR, PTR, 64, 64, 1024, 1024, 1024, 0, 1, PTR,
        _lib.lib().fbn_gemm_slabs_size(64, 64, 1024) - 4, None, 0, gr.INT_MAX, None, 0, gr.INT_MAX,
        ctypes.byref(ctypes.c_int(0)), None), "ws >= fbn_gemm_slabs_size"),
]


@pytest.mark.parametrize("fn,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refused_on_the_host_before_any_launch(fn, msg):
    """Each argument check of gemm_impl / fbn_gemm_split / fbn_gemm_slabs below returns before the plan is made and
    before any launch (read in gemm.hip), so a dummy address is never touched and no GPU is needed."""
    with pytest.raises(RuntimeError, match="code 1") as e:
        fn()
    assert msg in str(e.value), str(e.value)
