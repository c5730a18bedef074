"""The float64 reference, the derived error bound, the case table and a plain-Python mirror of the host
planning shared by the GEMM tests (test_gemm_ref_host.py, test_gpu_gemm.py).

Plain torch; no project kernel and no library call is involved.  csrc/gemm.hip computes

    C[m][rC(n)] = sum_k A(m,k) B(k,n) + bias[n] + beta C[m][rC(n)]

from operands in one of four storage layouts ("N" A[m*lda+k] / "T" A[k*lda+m]; "T" B[n*ldb+rB(k)] / "N"
B[k*ldb+rB(n)]), rB / rC two-segment remaps i -> i + (i < seg ? off0 : off1).  ``reference`` gathers the
operands out of the very storage tensors the kernel is given (so strides, remaps, split operands and image
offsets are the reference's own reading of that documentation) and returns C_ref and S in float64, S the same
expression with every term replaced by its absolute value: the scale of the summands.

Two kinds of input (``make_inputs``):
  "int"   operands, bias and C0 drawn from {-3..3}, beta in {0, 1, 2}: every product and every partial sum is
          exact in bf16 and fp32 (|sum| <= 9 K + 9 < 2^24 for every K of the table), so the result does not
          depend on accumulation order, tile, split or ring depth, on any path (the lo planes / lo images of
          the split-bf16 modes are exactly zero): C must equal C_ref bit for bit, and fbn_gemm_bf16out's C
          must equal C_ref rounded once to bf16.
  "real"  randn operands (rounded to bf16 where they are bf16 in memory), K <= 256 only.  Elementwise bound
              |C - C_ref| <= (c_prod + (K + 2) 2^-24) S
          (K + 2) 2^-24: fp32 accumulation of K products in any order plus the bias and beta adds;
          c_prod = 0 for fp32 operands (exact fp32 products) and for bf16 operands (bf16 x bf16 is exact in
          fp32; where the kernel rounds an fp32 operand to bf16 on its LDS store -- bf16 = 1 with an fp32
          operand -- the reference rounds it first with torch's round-to-nearest-even .bfloat16());
          c_prod = 3 x 2^-18 for split-bf16 x3 (bf16 = 2, fbn_gemm_s3): x = hi + lo + e, |lo| <= 2^-9 |x|,
          |e| <= 2^-18 |x|; per product the error terms e_a b, a e_b and the dropped lo_a lo_b are each
          <= 2^-18 |a b|.
          fbn_gemm_bf16out rounds the fp32 result c once more, to 8 significant bits (unit roundoff 2^-8):
          + 2^-8 |c| <= 2^-8 (|C_ref| + the bound above).
          Above K = 256 the worst-case bound stops separating one wrong term from rounding (K = 4096: a
          dropped product is at about the bound; K = 240: about 170x above it), so larger K run "int" only.

Canaries: C is [M + 2][ldc], ldc > N (or the remapped width), prefilled with C0 where beta != 0 and with a NaN
of a fixed bit pattern everywhere else; the ld gaps of A and B and the B columns rB skips hold NaN.

The plan mirror (``plan_gemm``, ``plan_dma16``, ``dma16_eligible``, ``resolve``) copies gemm.hip's host planning
so that every case can name the path it is meant to reach (``Case.path``) and the host test can prove it:
kernel family, tile, waves, ring depth, split after gemm_impl's per / split rounding, reduce kernel.

What each group of rows is there for (row names are the prefixes of the case ids):
  g128x128 / g128x64 / g64x128 / g64x64   launch_sel / launch_split: the four tiles of the generic kernel, ragged last
                      tiles, a K tail; g64x64: all six operand-type variants of launch_types in all four layouts
  gwide / gwide16     gemm_splitk_reduce4_wide (split 32, and its threshold 16) against a reference
  gsplit              gemm_splitk_reduce4; a K tail inside a split (bk 32), bf16 compute at split 2 (bk 64)
  gscalar             the scalar gemm_splitk_reduce (N % 4 != 0)
  gdv16               production: the d = 16 bilinear dV, N = K = 16, both operands bf16, beta = 1
  grbk / grbn         production: rB on k (k-contiguous loader) and on n (k-major loader), ldb = 336
  grc*                a remapped C through the epilogue and each non-stats reduce
  stats-*             the statistics from the generic epilogue, gemm_splitk_reduce_stats and the DMA 8-wave tile
  d*                  launch_dma16_sel: 8 waves on 128x128 and 64x128 (and ragged M), 4 waves on 64x64, rings of 2
                      and 4, the 4-deep ring with 1 / 2 / 3 K steps, split 2 / 4 / 8; -c16: fbn_gemm_bf16out
  s3-*                fbn_gemm_s3: one, two (a chunk across two K-segments) and sixteen K chunks
  a2-* / b2-*         fbn_gemm_split and slab mode against float64: a split-K chunk straddling kseg, A2 / B2 with
                      their own row strides, the mlp.0.weight remap of C
every case: lda / ldb / ldc larger than the extents (except where production's value is the point), NaN in the
gaps, canaries around C, a poisoned and guarded workspace; mixed operand types: the a16 / b16 variants.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

INT_MAX = 0x7FFFFFFF
NO_REMAP = (INT_MAX, 0, 0)
U = 2.0 ** -24
C_X3 = 3 * 2.0 ** -18
CANARY_F32 = 0x7FC0BEEF                                                            # a quiet NaN with a payload
CANARY_BF16 = 0x7FC5                                                               # likewise, bf16
REAL_MAX_K = 256
LAYOUTS = [(False, True), (False, False), (True, False), (True, True)]              # (transA, transB)


def wa_remap(d: int):
    """compact MLP-input column -> mlp.0.weight column (the production remap: skips V_0 and the (0, j) pairs)"""
    return (5 * d, d, 6 * d)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def pad_ld(extent: int) -> int:
    """a row stride larger than the extent, a multiple of 8 (16-byte rows of bf16)"""
    return cdiv(extent, 8) * 8 + 8


def remap_index(rm, n: int, device=None) -> torch.Tensor:
    i = torch.arange(n, device=device)
    return i + torch.where(i < rm[0], rm[1], rm[2])


def remap_extent(rm, n: int) -> int:
    return n if n == 0 else int(remap_index(rm, n).max()) + 1


# ----------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    id: str
    entry: str            # gemm | split | bf16out | s3 | slabs
    M: int
    N: int
    K: int                # the logical K (fbn_gemm_s3: K0; the kernel runs 3 K0)
    tA: bool
    tB: bool
    types: str            # f32 | bf1 | x3 | a16 | b16 | ab16   (bf1: bf16 compute on fp32 operands; x3: bf16 = 2)
    path: str             # the dispatch path the case is meant to reach (resolve(case)["path"])
    lda: int = 0          # 0: pad_ld(extent)
    ldb: int = 0
    ldc: int = 0
    rB: Tuple[int, int, int] = NO_REMAP
    rC: Tuple[int, int, int] = NO_REMAP
    beta: float = 0.0
    bias: bool = False
    stats: bool = False
    kseg: int = 0         # > 0: A = [A | A2] along K
    nseg: int = 0         # > 0: B = [B | B2] along N

    @property
    def bf16(self) -> int:
        return {"f32": 0, "x3": 2}.get(self.types, 1)

    @property
    def a16(self) -> bool:
        return self.types in ("a16", "ab16")

    @property
    def b16(self) -> bool:
        return self.types in ("b16", "ab16")

    @property
    def kk(self) -> int:
        """the K the kernel runs"""
        return 3 * self.K if self.entry == "s3" else self.K

    @property
    def real_ok(self) -> bool:
        return self.K <= REAL_MAX_K

    @property
    def c_prod(self) -> float:
        return C_X3 if (self.types == "x3" or self.entry == "s3") else 0.0

    # storage geometry -------------------------------------------------------------------------
    @property
    def a_cols(self) -> int:
        return self.M if self.tA else (self.kseg or self.K)

    @property
    def b_cols(self) -> int:
        return remap_extent(self.rB, self.K) if self.tB else remap_extent(self.rB, self.nseg or self.N)

    @property
    def LDA(self) -> int:
        return self.lda or pad_ld(self.a_cols)

    @property
    def LDB(self) -> int:
        return self.ldb or pad_ld(self.b_cols)

    @property
    def LDA2(self) -> int:
        return pad_ld(self.K - self.kseg)

    @property
    def LDB2(self) -> int:
        return pad_ld(self.N - self.nseg)

    @property
    def LDC(self) -> int:
        if self.entry == "slabs":
            return self.N
        return self.ldc or pad_ld(remap_extent(self.rC, self.N))

    @property
    def c_rows(self) -> int:
        return self.M if self.entry == "slabs" else self.M + 2


def _lay(tA, tB):
    return ("T" if tA else "N") + ("T" if tB else "N")


def _betas(i):      # spread beta / bias over a row's variants: the fast epilogue needs beta = 0, the slow one not
    return (0.0, 1.0, 2.0, 0.0)[i % 4], (True, False, True, False)[(i // 2 + i) % 4]


def _generic_rows() -> List[Case]:
    out: List[Case] = []

    def row(name, M, N, K, types, path32, path64, layouts=LAYOUTS, **kw):
        for t in types:
            for i, (tA, tB) in enumerate(layouts):
                beta, bias = _betas(i + len(out))
                p = path64 if t in ("bf1", "a16", "b16", "ab16") else path32
                out.append(Case(f"{name}-{t}-{_lay(tA, tB)}", "gemm", M, N, K, tA, tB, t, p,
                                **{"beta": beta, "bias": bias, **kw}))

    every = ("f32", "bf1", "x3", "a16", "b16", "ab16")
    # the three big tiles: 16-17 M outputs at K = 40 (a K tail of 8; bk = 64: one ragged K tile)
    row("g128x128", 4096, 4096, 40, ("f32", "x3"), "generic:128x128:split1:none", "generic:128x128:split1:none")
    row("g128x64", 32768, 200, 40, ("f32", "ab16"), "generic:128x64:split1:none", "generic:128x64:split1:none")
    row("g64x128", 200, 32768, 40, ("f32", "bf1"), "generic:64x128:split1:none", "generic:64x128:split1:none")
    # ragged in M, N and K together
    row("g64x64", 70, 72, 36, every, "generic:64x64:split1:none", "generic:64x64:split1:none")
    # many slabs over a small C: the wide reduce, and its threshold split = 16 (both-bf16 would take the DMA kernel)
    row("gwide", 64, 64, 4096, ("f32", "x3", "bf1", "a16", "b16"), "generic:64x64:split32:reduce4_wide",
        "generic:64x64:split16:reduce4_wide")
    row("gwide16", 64, 64, 2048, ("f32", "bf1"), "generic:64x64:split16:reduce4_wide", "generic:64x64:split8:reduce4")
    # split 4 (bk 32; last chunk 232 long: a K tail inside a split) / split 2 (bk 64)
    row("gsplit", 200, 136, 1000, every, "generic:64x64:split4:reduce4", "generic:64x64:split2:reduce4")
    # N % 4 != 0: the scalar reduce; NT with ldb = K is the issue's form (no gap in B)
    row("gscalar", 70, 70, 1000, ("f32", "x3", "ab16"), "generic:64x64:split4:reduce", "generic:64x64:split2:reduce",
        layouts=[(False, False), (True, False), (True, True)])
    row("gscalar", 70, 70, 1000, ("f32", "ab16"), "generic:64x64:split4:reduce", "generic:64x64:split2:reduce",
        layouts=[(False, True)], ldb=1000)
    # production: the d = 16 bilinear dV (both operands bf16, a quarter of one K tile, beta = 1, no gaps)
    out.append(Case("gdv16-ab16-NT", "gemm", 185, 16, 16, False, True, "ab16", "generic:64x64:split1:none",
                    lda=16, ldb=16, ldc=16, beta=1.0))
    out.append(Case("gdv16-f32-NT", "gemm", 185, 16, 16, False, True, "f32", "generic:64x64:split1:none",
                    lda=16, ldb=16, ldc=16, beta=1.0))
    # production: rB on k (the fp32 layer-1 forward, k-contiguous B loader) and on n (its dgrad, k-major loader)
    row("grbk", 100, 64, 240, ("f32", "bf1", "x3", "a16"), "generic:64x64:split1:none", "generic:64x64:split1:none",
        layouts=[(False, True), (True, True)], rB=wa_remap(16), ldb=336)
    row("grbn", 100, 240, 72, ("f32", "bf1", "x3", "a16"), "generic:64x64:split1:none", "generic:64x64:split1:none",
        layouts=[(False, False), (True, False)], rB=wa_remap(16), ldb=336)
    # a remapped C through the generic epilogue and through each non-stats reduce that takes one
    row("grc", 70, 72, 36, ("f32",), "generic:64x64:split1:none", "", layouts=[(False, True)], rC=(40, 8, 24))
    row("grcsplit", 200, 136, 1000, ("f32",), "generic:64x64:split4:reduce4", "", layouts=[(True, False)],
        rC=(40, 8, 24))
    row("grcwide", 64, 64, 4096, ("f32",), "generic:64x64:split32:reduce4_wide", "", layouts=[(False, False)],
        rC=(40, 8, 24))
    row("grcscalar", 70, 70, 1000, ("f32",), "generic:64x64:split4:reduce", "", layouts=[(False, True)],
        rC=(40, 8, 24))
    return out


def _stats_rows() -> List[Case]:
    out = []
    for t, (tA, tB) in (("f32", (False, True)), ("ab16", (True, False))):
        out.append(Case(f"stats-epi-{t}-{_lay(tA, tB)}", "gemm", 200, 72, 36, tA, tB, t, "generic:64x64:split1:none",
                        bias=True, stats=True))
    for t, p, (tA, tB) in (("f32", "generic:64x64:split4:reduce_stats", (False, True)),
                           ("bf1", "generic:64x64:split2:reduce_stats", (True, True))):
        out.append(Case(f"stats-red-{t}-{_lay(tA, tB)}", "gemm", 200, 136, 1000, tA, tB, t, p, bias=True, stats=True))
    for tA, tB in ((False, True), (True, False)):
        out.append(Case(f"stats-dma-ab16-{_lay(tA, tB)}", "gemm", 4096 - 24, 1024, 64, tA, tB, "ab16",
                        "dma:128x128:w8:ring2:split1:none", bias=True, stats=True))
    return out


DMA_ROWS = [   # name, M, N, K, path (fbn_gemm), path with bf16 C (never split) or None
    ("d128x128", 4096, 1024, 64, "dma:128x128:w8:ring2:split1:none", "dma:128x128:w8:ring2:split1:none"),
    ("d128x128r", 4096 - 24, 1024, 64, "dma:128x128:w8:ring2:split1:none", None),
    ("d64x128", 2048, 1024, 64, "dma:64x128:w8:ring2:split1:none", "dma:64x128:w8:ring2:split1:none"),
    ("d64x128r", 2048 - 24, 1024, 64, "dma:64x128:w8:ring2:split1:none", None),
    ("d64x64big", 32768, 64, 64, "dma:64x64:w4:ring2:split1:none", "dma:64x64:w4:ring2:split1:none"),
    ("d128split", 512, 512, 1024, "dma:128x128:w8:ring4:split8:reduce4", None),
    ("dtiny1", 64, 64, 64, "dma:64x64:w4:ring4:split1:none", None),
    ("dtiny2", 64, 64, 128, "dma:64x64:w4:ring4:split1:none", None),
    ("dtiny3", 64, 64, 192, "dma:64x64:w4:ring4:split1:none", None),
    ("dtinysplit", 64, 64, 1024, "dma:64x64:w4:ring4:split8:reduce4", None),
    ("dsplit4", 320, 320, 1024, "dma:64x64:w4:ring2:split4:reduce4", None),
    ("dragged", 200, 136, 256, "dma:64x64:w4:ring4:split2:reduce4", "dma:64x64:w4:ring4:split1:none"),
]


def _dma_rows() -> List[Case]:
    out: List[Case] = []
    for name, M, N, K, path, path16 in DMA_ROWS:
        for i, (tA, tB) in enumerate(LAYOUTS):
            beta, bias = _betas(i + len(out))
            out.append(Case(f"{name}-{_lay(tA, tB)}", "gemm", M, N, K, tA, tB, "ab16", path, beta=beta, bias=bias))
            if path16:
                out.append(Case(f"{name}-c16-{_lay(tA, tB)}", "bf16out", M, N, K, tA, tB, "ab16", path16))
    for M, N, K0, path in ((64, 64, 64, "dma:64x64:w4:ring2:split1:none"),
                           (200, 136, 128, "dma:64x64:w4:ring2:split2:reduce4"),
                           (512, 512, 1024, "dma:128x128:w8:ring2:split16:reduce4")):
        for tA, tB in LAYOUTS:
            for beta in (0.0, 1.0):
                out.append(Case(f"s3-{M}x{N}x{K0}-b{int(beta)}-{_lay(tA, tB)}", "s3", M, N, K0, tA, tB, "ab16", path,
                                beta=beta))
    return out


def _split_rows() -> List[Case]:
    out: List[Case] = []
    a2 = ((100, 512, 1920, 640, "dma:64x64:w4:ring4:split8:"),    # chunks of 256: chunk 2 straddles kseg
          (72, 64, 384, 128, "dma:64x64:w4:ring4:split2:"),       # chunks of 192: the first straddles
          (64, 64, 256, 128, "dma:64x64:w4:ring4:split2:"))       # chunks of 128: none does
    for M, N, K, kseg, p in a2:
        for i, tB in enumerate((True, False)):
            out.append(Case(f"a2-{M}x{N}x{K}-{_lay(False, tB)}", "split", M, N, K, False, tB, "ab16", p + "reduce4",
                            kseg=kseg, beta=float(i), bias=not i))
            out.append(Case(f"a2-{M}x{N}x{K}-slabs-{_lay(False, tB)}", "slabs", M, N, K, False, tB, "ab16",
                            p + "slabs", kseg=kseg))
    b2 = ((512, 1920, 1024, 640, "dma:128x128:w8:ring2:split4:", wa_remap(128), 21 * 128),
          (64, 256, 128, 128, "dma:64x64:w4:ring4:split1:", NO_REMAP, 0))
    for M, N, K, nseg, p, rC, ldc in b2:
        for i, tA in enumerate((True, False)):
            red = "none" if p.endswith("split1:") else "reduce4"
            out.append(Case(f"b2-{M}x{N}x{K}-{_lay(tA, False)}", "split", M, N, K, tA, False, "ab16", p + red,
                            nseg=nseg, rC=rC, ldc=ldc, beta=float(2 * i), bias=bool(i)))
            out.append(Case(f"b2-{M}x{N}x{K}-slabs-{_lay(tA, False)}", "slabs", M, N, K, tA, False, "ab16",
                            p + "slabs", nseg=nseg))
    return out


CASES: List[Case] = _generic_rows() + _stats_rows() + _dma_rows() + _split_rows()
assert len({c.id for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------ plan mirror
def plan_gemm(M, N, K, bk):
    for bm, bn in ((128, 128), (128, 64), (64, 128), (64, 64)):
        if (bm == 128 and M < 256) or (bn == 128 and N < 256):
            continue
        if cdiv(M, bm) * cdiv(N, bn) >= 1024:
            return dict(bm=bm, bn=bn, split=1, waves=4, stages=0)
    tiles = cdiv(M, 64) * cdiv(N, 64)
    s = 1
    while tiles * s < 1024 and K // (s * 2) >= 4 * bk and s < 64:
        s *= 2
    return dict(bm=64, bn=64, split=s, waves=4, stages=0)


def plan_dma16(M, N, K):
    t64 = cdiv(M, 64) * cdiv(N, 64)
    if t64 >= 512:
        if N >= 1024 and cdiv(M, 128) * cdiv(N, 128) >= 256:
            return dict(bm=128, bn=128, split=1, waves=8, stages=0)
        if N >= 128:
            return dict(bm=64, bn=128, split=1, waves=8, stages=0)
        return dict(bm=64, bn=64, split=1, waves=4, stages=0)
    p = dict(bm=128, bn=128, split=1, waves=8, stages=0) if (M >= 512 and N >= 512) else \
        dict(bm=64, bn=64, split=1, waves=4, stages=0)
    tiles = cdiv(M, p["bm"]) * cdiv(N, p["bn"])
    target = 512 if p["bm"] == 128 else 256
    tiny = tiles <= 16
    min_k = 128 if tiny else 256
    while p["split"] < 64 and tiles * p["split"] * 2 <= target and K // (p["split"] * 2) >= min_k:
        p["split"] *= 2
    if tiny:
        p["stages"] = 4
    return p


def slab_split(M, N, K):
    per = cdiv(cdiv(K, plan_dma16(M, N, K)["split"]), 64) * 64
    return cdiv(K, per) if K > 0 else 1


def workspace_size(M, N, K, bf16):
    """fbn_gemm_workspace_size: the larger split of the two kernels' plans (before gemm_impl's rounding)"""
    s = plan_gemm(M, N, K, 64 if bf16 == 1 else 32)["split"]
    if bf16:
        s = max(s, plan_dma16(M, N, K)["split"])
    return s * M * N * 4 if s > 1 else 0


def dma16_eligible(c: Case) -> bool:
    return bool(c.bf16 and c.a16 and c.b16 and c.rB[0] == INT_MAX and c.kk % 64 == 0 and c.LDA % 8 == 0
                and c.LDB % 8 == 0 and (not c.tA or c.M % 8 == 0) and (c.tB or c.N % 8 == 0))


def ws_bytes(c: Case) -> int:
    """what the caller allocates: fbn_gemm_slabs_size for slab mode, else fbn_gemm_workspace_size"""
    if c.entry == "slabs":
        return slab_split(c.M, c.N, c.K) * c.M * c.N * 4
    if c.entry == "bf16out":
        return 0
    return workspace_size(c.M, c.N, c.kk, c.bf16)


def resolve(c: Case) -> dict:
    """the launch gemm_impl makes for the case, given the workspace ws_bytes(c)"""
    K = c.kk
    dma = dma16_eligible(c)
    bk = 64 if c.bf16 == 1 else 32
    p = plan_dma16(c.M, c.N, K) if dma else plan_gemm(c.M, c.N, K, bk)
    ws = ws_bytes(c)
    if c.entry == "slabs":
        p["split"] = slab_split(c.M, c.N, K)
    if p["split"] > 1 and (c.entry == "bf16out" or ws < p["split"] * c.M * c.N * 4):
        p["split"] = 1
    per = cdiv(cdiv(K, p["split"]), bk) * bk
    p["split"] = cdiv(K, per) if K > 0 else 1
    if c.stats and p["split"] == 1 and not (dma and p["waves"] == 8 and p["bm"] == 128):
        p["bm"] = 64
    p["kchunk"] = per
    rC = c.rC
    v4 = c.N % 4 == 0 and c.LDC % 4 == 0 and (rC[0] == INT_MAX or rC[0] % 4 == 0) and rC[1] % 4 == 0 and rC[2] % 4 == 0
    if c.entry == "slabs":
        red = "slabs"
    elif p["split"] == 1:
        red = "none"
    elif c.stats:
        red = "reduce_stats"
    elif v4:
        red = "reduce4_wide" if (p["split"] >= 16 and c.M * c.N // 4 < 65536) else "reduce4"
    else:
        red = "reduce"
    p["reduce"] = red
    p["kernel"] = "dma" if dma else "generic"
    if dma:
        ring = 2 if c.entry == "s3" else (p["stages"] or 2)        # FBN_DMA_STAGES = 2; the S3 kernels: two stages
        p["path"] = f"dma:{p['bm']}x{p['bn']}:w{p['waves']}:ring{ring}:split{p['split']}:{red}"
    else:
        p["path"] = f"generic:{p['bm']}x{p['bn']}:split{p['split']}:{red}"
    return p


# ------------------------------------------------------------------------------------------------ inputs
@dataclass
class Inputs:
    A: torch.Tensor                     # storage; fbn_gemm_s3: [2][rows][lda] (hi, lo)
    B: torch.Tensor
    A2: Optional[torch.Tensor]
    B2: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    C0: torch.Tensor                    # [c_rows][ldc] f32 (bf16out: bf16), canaries outside the read set


def _draw(shape, kind, gen, device):
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=gen, device=device).float()
    return torch.randn(shape, generator=gen, device=device)


def _store(x, ld, rm, dtype):
    """x [rows][cols] at st[r][rm(c)] of a NaN-filled [rows][ld]"""
    st = torch.full((x.shape[0], ld), float("nan"), dtype=dtype, device=x.device)
    st[:, remap_index(rm, x.shape[1], x.device)] = x.to(dtype)
    return st


def canary_fill(shape, dtype, device):
    if dtype == torch.bfloat16:
        return torch.full(shape, CANARY_BF16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full(shape, CANARY_F32, dtype=torch.int32, device=device).view(torch.float32)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else torch.int64)


def written_mask(c: Case, device=None) -> torch.Tensor:
    m = torch.zeros((c.c_rows, c.LDC), dtype=torch.bool, device=device)
    m[:c.M, remap_index(c.rC, c.N, device)] = True
    return m


def make_inputs(c: Case, kind: str, device="cpu", seed: int = 0) -> Inputs:
    gen = torch.Generator(device=device).manual_seed(1000 + seed)
    a = _draw((c.M, c.K), kind, gen, device)
    b = _draw((c.K, c.N), kind, gen, device)
    ta = torch.bfloat16 if c.a16 else torch.float32
    tb = torch.bfloat16 if c.b16 else torch.float32
    A2 = B2 = None
    if c.entry == "s3":
        def images(x, ld):
            hi = x.bfloat16()
            lo = (x - hi.float()).bfloat16()
            return torch.stack([_store(hi, ld, NO_REMAP, torch.bfloat16), _store(lo, ld, NO_REMAP, torch.bfloat16)])
        A = images(a.T if c.tA else a, c.LDA)
        B = images(b.T if c.tB else b, c.LDB)
    else:
        if c.kseg:
            A, A2 = _store(a[:, :c.kseg], c.LDA, NO_REMAP, ta), _store(a[:, c.kseg:], c.LDA2, NO_REMAP, ta)
        else:
            A = _store(a.T if c.tA else a, c.LDA, NO_REMAP, ta)
        if c.nseg:
            B, B2 = _store(b[:, :c.nseg], c.LDB, NO_REMAP, tb), _store(b[:, c.nseg:], c.LDB2, NO_REMAP, tb)
        else:
            B = _store(b.T if c.tB else b, c.LDB, c.rB, tb)
    bias = _draw((c.N,), kind, gen, device) if c.bias else None
    tc = torch.bfloat16 if c.entry == "bf16out" else torch.float32
    C0 = canary_fill((c.c_rows, c.LDC), tc, device)
    if c.beta != 0.0:
        c0 = _draw((c.M, c.N), kind, gen, device)
        C0[:c.M, remap_index(c.rC, c.N, device)] = c0
    return Inputs(A, B, A2, B2, bias, C0)


# --------------------------------------------------------------------------------------------- reference
def logical_a(c: Case, A, A2=None, kseg=None) -> torch.Tensor:
    """A(m, k) [M][K] out of the storage, as gemm.hip documents the layouts"""
    kseg = c.kseg if kseg is None else kseg
    if c.kseg:
        k2 = torch.arange(c.K - kseg, device=A.device) % (c.K - c.kseg)     # kseg != c.kseg: a test's wrong reading
        return torch.cat([A[:c.M, :kseg], A2[:c.M][:, k2]], 1)
    return A[:c.K, :c.M].T if c.tA else A[:c.M, :c.K]


def logical_b(c: Case, B, B2=None, rB=None) -> torch.Tensor:
    """B(k, n) [K][N]"""
    rB = c.rB if rB is None else rB
    if c.nseg:
        return torch.cat([B[:c.K, :c.nseg], B2[:c.K, :c.N - c.nseg]], 1)
    if c.tB:
        return B[:c.N][:, remap_index(rB, c.K, B.device)].T
    return B[:c.K][:, remap_index(rB, c.N, B.device)]


def logical_c(c: Case, C, rC=None) -> torch.Tensor:
    rC = c.rC if rC is None else rC
    return C[:c.M][:, remap_index(rC, c.N, C.device)]


def operands64(c: Case, A, B, swap_lo: bool = False):
    """the two logical operands in float64, as the kernel's arithmetic sees them (see the module docstring)"""
    A, A2 = A if isinstance(A, tuple) else (A, None)
    B, B2 = B if isinstance(B, tuple) else (B, None)
    if c.entry == "s3":
        lo_a, lo_b = (B[1], A[1]) if swap_lo else (A[1], B[1])
        a = logical_a(c, A[0]).double() + logical_a(c, lo_a).double()
        b = logical_b(c, B[0]).double() + logical_b(c, lo_b).double()
        return a, b
    a, b = logical_a(c, A, A2), logical_b(c, B, B2)
    if c.bf16 == 1:          # fp32 operands are rounded to bf16 on the LDS store (bf16 ones: a no-op)
        a, b = a.bfloat16(), b.bfloat16()
    return a.double(), b.double()


def reference(c: Case, A, B, bias, C0, swap_lo: bool = False):
    """(C_ref, S) [M][N] float64.  A / B: the storage tensors, (A, A2) / (B, B2) for split operands, the
    [2][rows][ld] (hi, lo) images for fbn_gemm_s3; C0: the C storage before the call (read where beta != 0).
    swap_lo (fbn_gemm_s3, equal storage shapes): A reads B's lo image and B reads A's -- a wrong reference."""
    a, b = operands64(c, A, B, swap_lo)
    ref = a @ b
    S = a.abs() @ b.abs()
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs()
    if c.beta != 0.0:
        c0 = logical_c(c, C0).double()
        ref = ref + c.beta * c0
        S = S + abs(c.beta) * c0.abs()
    return ref, S


def bound(c: Case, C_ref, S):
    bd = (c.c_prod + (c.K + 2) * U) * S
    if c.entry == "bf16out":
        bd = bd + 2.0 ** -8 * (C_ref.abs() + bd)
    return bd


def check(c: Case, kind: str, C, C0, C_ref, S):
    """(ok, worst err / bound of a real case or None, message).  C: the C storage after the call (slab mode: the
    float64 sum of the slabs, [M][N])."""
    dev = C.device
    mask = written_mask(c, dev)
    if C.shape != mask.shape:
        return False, None, f"C has shape {tuple(C.shape)}"
    if c.entry != "slabs" and not torch.equal(bits(C)[~mask], bits(C0)[~mask]):
        bad = ((bits(C) != bits(C0)) & ~mask).nonzero()
        return False, None, f"{len(bad)} elements outside the written set changed, first at {bad[0].tolist()}"
    got = logical_c(c, C)
    if not bool(torch.isfinite(got).all()):
        bad = (~torch.isfinite(got)).nonzero()
        return False, None, f"{len(bad)} non-finite elements inside the written set, first at {bad[0].tolist()}"
    if kind == "int":
        want = C_ref.to(torch.bfloat16) if c.entry == "bf16out" else C_ref
        same = got.double() == want.double()
        if not bool(same.all()):
            bad = (~same).nonzero()
            m, n = bad[0].tolist()
            return False, None, (f"{len(bad)} of {same.numel()} elements differ from the exact result, first at "
                                 f"({m}, {n}): {got[m, n].item()} != {want[m, n].item()}")
        return True, None, ""
    err = (got.double() - C_ref).abs()
    bd = bound(c, C_ref, S)
    ratio = float((err / bd.clamp_min(1e-300)).max())
    over = err > bd
    if bool(over.any()):
        m, n = over.nonzero()[0].tolist()
        return False, ratio, (f"{int(over.sum())} elements over the bound, worst err / bound {ratio:.3g}, first at "
                              f"({m}, {n}): err {err[m, n].item():.3g} bound {bd[m, n].item():.3g}")
    return True, ratio, ""
