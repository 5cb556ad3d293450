"""A model of what the fused SetAbstraction kernels compute (csrc/sa_mlp_x3.hip, csrc/sa_mlp16.hip), for
the tests: rigorous per-element forward bounds with the kernels' OWN scaling groups, a bit-level emulation
of the documented h3 arithmetic (csrc/h3.hpp) with mutants, and weight / input families that leave the
benign fresh-init regime.  numpy only; TEST INFRASTRUCTURE.

h3 in one paragraph: an fp32 value v of a scaling group whose maximum is below 2^e is scaled by 2^(14 - e)
(exact) and split as hi = fp16(v S), lo = fp16(v S - hi), both RNE.  With fp16's unit roundoff 2^-11 and
subnormal step 2^-24 the residual r = v S - hi - lo obeys |r| <= max(2^-22 |v S|, 2^-25) and the low piece
|lo| <= max(2^-11 |v S|, 2^-25) + |r|.  A product keeps ah bh + ah bl + al bh and drops
al bl + ar b + (ah + al) br; the kept products are exact in fp32 and are accumulated in fp32 (3K + 4 adds),
the sum is unscaled by an exact power of two in one fma with the bias.

The scaling groups of the SA kernels:
  weights       per layer, exponent s in the packed image's tail (max |W| 2^s < 2^14)
  layer 2 in    per 16-row tile of one centre: e2 = exp_of_bits(tile max of y1), floor kEmin = -100
  layer 3 in    per 16-row tile, NOT from the data: e3 = exp_of_bits((colsum2 2^e2 + bmax2)(1 + 2^-10)),
                colsum2 = max_c sum_k |W2[k][c]| and bmax2 = max |b2| from the tail (bound_exp3)
"""
import numpy as np

U24 = 2.0 ** -24
KEMIN, KEMAX = -100, 128
TILE = 16            # rows of one scaling tile
H11 = 2.0 ** -11     # fp16 unit roundoff
R22 = 2.0 ** -22     # the two-piece residual, relative
SUB = 2.0 ** -25     # half the fp16 subnormal step: the absolute residual of scaled values, and of lo
MUTANTS = ("drop_ah_bl", "drop_al_bh", "trunc_l3_lo")
# (xyz_level, c1, c2, c3, nsample): csrc/sa_shapes.hpp LIDAR_SA_SHAPES, with the radius of the configuration's branch
SHAPES = [(True, 32, 32, 64, 16), (True, 64, 64, 128, 32), (True, 64, 96, 128, 128),
          (False, 64, 64, 128, 32), (False, 128, 128, 256, 64), (False, 128, 128, 256, 128)]
RADII = {(True, 32, 32, 64, 16): 0.1, (True, 64, 64, 128, 32): 0.2, (True, 64, 96, 128, 128): 0.4,
         (False, 64, 64, 128, 32): 0.2, (False, 128, 128, 256, 64): 0.4, (False, 128, 128, 256, 128): 0.8}
FAMILIES = ["fresh", "bn_spread8", "bn_spread16", "sparse", "loose_bound12", "outlier_row", "tiny", "huge"]
CFEAT = 61           # feature channels of the single-kernel feature-level cases (3 + 61 = 64 input columns)
PLANT = 136          # the planted run of points (sparse: copies of one point with zero features): > 128 = max nsample
C0 = PLANT - 3       # the centres are points C0 .. C0 + M - 1: three planted ones, then ordinary points


def shape_id(s):
    return ("xyz" if s[0] else "pre") + "-" + "-".join(str(int(v)) for v in s[1:])


# ---------------------------------------------------------------------------------- the kernels' scaling
def exp_of(m):
    """h3.hpp exp_of_bits on non-negative float32 values: e with m < 2^e, clamped to [kEmin, kEmax]."""
    b = np.asarray(m, dtype=np.float32).view(np.uint32).astype(np.int64) & 0x7fffffff
    e8 = b >> 23
    return np.clip(np.where(e8 == 0, KEMIN, e8 - 126), KEMIN, KEMAX)


def read_tail(image):
    """X3Tail of pack_branch_x3's image: its last 16 bytes (int32 s2, s3; float colsum2, bmax2)."""
    t = np.ascontiguousarray(image).view(np.uint8)[-16:].copy()
    s2, s3 = (int(v) for v in t[:8].view(np.int32))
    colsum2, bmax2 = t[8:].view(np.float32)
    return {"s2": s2, "s3": s3, "colsum2": np.float32(colsum2), "bmax2": np.float32(bmax2)}


def packed_x3(layers, xyz_level):
    """pack_branch_x3's image with the packer's envelope warning silenced: the families here leave the
    envelope on purpose (tests/test_h3_model_cpu.py checks the warning itself)."""
    import warnings
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return pn.pack_branch_x3(layers, xyz_level)


def packed_tail(layers, xyz_level):
    return read_tail(packed_x3(layers, xyz_level))


def bound_value(tail, e2):
    """sa_mlp_x3.hip bound_exp3's bound on a tile's |y2|, in its float32 arithmetic (colsum2 2^e2 is exact,
    so a contracted fma gives the same bits)."""
    with np.errstate(over="ignore"):
        p2 = np.exp2(np.asarray(e2, dtype=np.float64)).astype(np.float32)
        return (tail["colsum2"] * p2 + tail["bmax2"]) * np.float32(1 + 2.0 ** -10)


def bound_exp3(tail, e2):
    return exp_of(bound_value(tail, e2))


def _tile_exp(amag):
    """Per row, the exponent of its 16-row tile: from the tile maximum of amag (>= the kernel's values),
    rounded up to float32, so never below the kernel's own exponent."""
    R = amag.shape[0]
    m = amag.reshape(R // TILE, -1).max(axis=1)
    m32 = np.nextafter(m.astype(np.float32), np.float32(np.inf))
    m32 = np.where(m == 0, np.float32(0), m32)
    return exp_of(m32)


def _pieces(mag, floor):
    """(|residual| bound, |lo| bound) of h3-split values of magnitude <= mag whose group's absolute
    floor (2^-25 in scaled units) is `floor`; both monotone in mag."""
    r = np.maximum(R22 * mag, floor)
    return r, np.maximum(H11 * mag, floor) + r


def _h3_layer_terms(amag, afloor, W, s_w, accumulate):
    """Error of one h3 GEMM, excluding propagation: the dropped products and the fp32 accumulation of the
    kept ones (3K + 4 correctly rounded adds, doubled for any internal rounding mode, as h3_forward_bound;
    accumulate = "f64": an exact accumulation, emulate_x3's, leaves 2^-50 of the kept products)."""
    Wm = np.abs(W)
    K = Wm.shape[0]
    rw, lw = _pieces(Wm, SUB * 2.0 ** -s_w)
    ra, la = _pieces(amag, afloor)
    dropped = la @ lw + ra @ Wm + (amag + ra) @ rw
    kept = (amag + ra) @ (Wm + rw)
    return dropped + (2 * (3 * K + 4) * U24 if accumulate == "fp32" else 2.0 ** -50) * kept


def _relu(y, e):
    """ReLU of an exact pre-activation y known to the kernel within e: (relu(y), the bound after it).  ReLU is
    1-Lipschitz, and where y + e <= 0 the kernel's value is <= 0 too: both outputs are exactly 0."""
    return np.maximum(y, 0.0), np.where(y + e <= 0, 0.0, e)


def _layer1(rows_or_PQ, layer, group, l1, k_terms):
    """Exact layer-1 output (before ReLU) and the kernel's error bound on it."""
    if l1 == "xyz":
        W, b = (np.asarray(a, np.float64) for a in layer)
        x = np.asarray(rows_or_PQ, np.float32).astype(np.float64)
        y = x @ W[:3] + b
        return y, 2 * k_terms(3) * U24 * (np.abs(x) @ np.abs(W[:3]) + np.abs(b))
    if l1 == "given":  # (exact layer-1 pre-activation, the bound on the kernel's): the caller's own layer-1 model
        y, e = rows_or_PQ
        return np.asarray(y, np.float64), np.asarray(e, np.float64)
    if l1 != "pre":
        raise ValueError("l1 must be 'xyz', 'pre' or 'given'")
    P, Q = rows_or_PQ
    P = np.asarray(P, np.float32).astype(np.float64)
    Q = np.asarray(Q, np.float32).astype(np.float64)
    if len(Q) != len(P):
        Q = np.repeat(Q, group, axis=0)
    y = P - Q  # the kernel: one fp32 subtraction of what it read
    return y, U24 * np.abs(y)


def x3_forward_bound(rows_or_PQ, layers, group, tail, *, l1, accumulate="fp32"):
    """A fused SA branch in h3 arithmetic (sa_x3_kernel / sa_x3_lean_kernel) with a rigorous per-element
    bound against the exact (float64) computation, using the kernels' own scaling groups (module docstring).

    l1 = "xyz": rows_or_PQ = the grouped offsets (R, 3) float32; layer 1 is the kernel's fp32 MFMA, K = 3.
    l1 = "pre": rows_or_PQ = (P rows gathered per grouped row (R, c1), Q rows per centre (R / group, c1)),
    the values the kernel read: layer 1 is relu(P - Q), one fp32 subtraction, and `layers[0]` is unused.
    l1 = "given": rows_or_PQ = (exact layer-1 pre-activation (R, c1), the bound on the kernel's error on it),
    for a caller that models P and Q itself (the backbone's levels, anchored on the previous level's output).
    tail: read_tail(pack_branch_x3(layers, ...)).  Per layer: e = the bound on |kernel input - exact input|;
    the output is off by e |W| (propagation) + the dropped products + the accumulation + the one rounding
    of the unscale-and-bias fma; ReLU and max-pool are 1-Lipschitz, and a ReLU that is surely off is exact.  Exponents are taken from |exact| + e,
    so they are never below the kernel's.  accumulate="f64" drops the fp32 accumulation term: the bound of
    emulate_x3, which sums exactly (the CPU tests hold the emulation and its mutants to that tighter bound).
    Returns (exact, bound), (R / group, c3) float64."""
    if accumulate not in ("fp32", "f64"):
        raise ValueError(accumulate)
    h, e = _relu(*_layer1(rows_or_PQ, layers[0], group, l1, lambda k: k + 4))
    e2 = None
    for j, (W, b) in enumerate(layers[1:]):
        Wd, bd = np.asarray(W, np.float64), np.asarray(b, np.float64)
        amag = h + e
        if j == 0:
            e2 = _tile_exp(amag)
            ea, sw = e2, tail["s2"]
        else:
            ea, sw = bound_exp3(tail, e2), tail["s3"]
        afloor = np.repeat(np.exp2(ea.astype(np.float64) - 39), TILE)[:, None]
        y = h @ Wd + bd
        t = e @ np.abs(Wd) + _h3_layer_terms(amag, afloor, Wd, sw, accumulate)
        h, e = _relu(y, t + 2 * U24 * (np.abs(y) + t) + U24 * np.abs(bd))
    C = h.shape[1]
    return h.reshape(-1, group, C).max(axis=1), e.reshape(-1, group, C).max(axis=1)


def f32_forward_bound(rows_or_PQ, layers, group, *, l1):
    """The same for sa_mlp16.hip: every layer on the native fp32 MFMA, 2 (K + 4) 2^-24 sum |a| |w| per layer
    (K + 1 correctly rounded adds with the bias, doubled as above), propagated the same way."""
    h, e = _relu(*_layer1(rows_or_PQ, layers[0], group, l1, lambda k: k + 4))
    for W, b in layers[1:]:
        Wd, bd = np.asarray(W, np.float64), np.asarray(b, np.float64)
        K = Wd.shape[0]
        y = h @ Wd + bd
        h, e = _relu(y, e @ np.abs(Wd) + 2 * (K + 4) * U24 * ((h + e) @ np.abs(Wd) + np.abs(bd)))
    C = h.shape[1]
    return h.reshape(-1, group, C).max(axis=1), e.reshape(-1, group, C).max(axis=1)


def dense_chain_bound(rows, layers, pool):
    """group_all's h3 chain (dense_x3s.hip: lidar_dense_h3p_f32 in modes 1, 1, 2) on fp32 rows (R, k) with a
    rigorous per-element bound, using the kernel's own row exponents.  Layer 1 splits a row under its
    running scale, exp_of_bits(row max) + 3 (three bits of headroom); every later layer reads the planes
    its producer wrote, split under the bound exponent of (colsum(W) 2^e_in + max |b|)(1 + 2^-10)
    (out_bound_exp: the rule of bound_exp3), not under the row's maximum.  Weights: per matrix,
    s = 14 - exp_of_bits(max |W|).  layers = [(W (k, c), b)] as the GEMMs read them (padded alike or not:
    zero rows and columns change nothing).  Returns (exact, bound), (R / pool, c_last) float64."""
    h = np.asarray(rows, np.float32).astype(np.float64)
    e = np.zeros_like(h)
    E = None
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    for j, (W, b) in enumerate(layers):
        Wd, bd = np.asarray(W, np.float64), np.asarray(b, np.float64)
        amag = np.abs(h) + e
        if j == 0:
            m = amag.max(axis=1)
            E = exp_of(np.where(m == 0, np.float32(0), np.nextafter(m.astype(np.float32), np.float32(np.inf)))) + 3
        else:
            Wp, bp = (np.asarray(a, np.float64) for a in layers[j - 1])
            prev = {"colsum2": up(np.abs(Wp).sum(axis=0).max()), "bmax2": up(np.abs(bp).max())}
            E = bound_exp3(prev, E - (3 if j == 1 else 0))
        s_w = 14 - int(exp_of(np.float32(np.abs(Wd).max())))
        y = h @ Wd + bd
        t = e @ np.abs(Wd) + _h3_layer_terms(amag, np.exp2(E.astype(np.float64) - 39)[:, None], Wd, s_w, "fp32")
        h, e = _relu(y, t + 2 * U24 * (np.abs(y) + t) + U24 * np.abs(bd))
    C = h.shape[1]
    return h.reshape(-1, pool, C).max(axis=1), e.reshape(-1, pool, C).max(axis=1)


# ---------------------------------------------------------------------------------- bit-level emulation
def _split(v32):
    """hi = fp16(v), lo = fp16(v - hi) of float32 values (RNE; v - hi is exact in fp32) -> float64 pieces."""
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _h3_matmul(a32, a_exp_rows, W, s_w, drop, no_lo):
    """The kept products of one h3 GEMM, summed in float64 (exact piece products), unscaled.  a_exp_rows:
    every row's scaling exponent; drop: a mutant's dropped product; no_lo: the activations' lo pieces cut."""
    with np.errstate(over="ignore"):
        sa = np.exp2(14.0 - a_exp_rows)[:, None].astype(np.float32)
        ah, al = _split(a32 * sa)
        wh, wl = _split(np.asarray(W, np.float32) * np.float32(2.0 ** s_w))
    if no_lo:
        al = np.zeros_like(al)
    acc = ah @ wh
    if drop != "drop_ah_bl":
        acc = acc + ah @ wl
    if drop != "drop_al_bh":
        acc = acc + al @ wh
    return acc * np.exp2(a_exp_rows - 14.0 - s_w)[:, None]


def emulate_x3(y1, layers, group, tail, mutant=None):
    """h3.hpp's arithmetic of layers 2-3 + max-pool on the layer-1 output y1 (R, c1) float32 (after ReLU),
    bit for bit in its splits, products and scaling groups; accumulation in float64 (the bound's
    accumulation term covers the kernel's fp32 order).  mutant: one of MUTANTS — drop the ah bl or the
    al bh product (both layers), or cut layer 3's lo fragments.  Returns (R / group, c3) float64."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    (W2, b2), (W3, b3) = layers[1], layers[2]
    y1 = np.ascontiguousarray(y1, dtype=np.float32)
    R = y1.shape[0]
    e2 = exp_of(y1.reshape(R // TILE, -1).max(axis=1))
    e2r = np.repeat(e2, TILE).astype(np.float64)
    acc = _h3_matmul(y1, e2r, W2, tail["s2"], mutant, False)
    y2 = np.maximum((acc + np.asarray(b2, np.float64)).astype(np.float32), np.float32(0))
    e3r = np.repeat(bound_exp3(tail, e2), TILE).astype(np.float64)
    acc = _h3_matmul(y2, e3r, W3, tail["s3"], mutant, mutant == "trunc_l3_lo")
    pooled = acc.reshape(-1, group, acc.shape[1]).max(axis=1)
    return np.maximum((pooled + np.asarray(b3, np.float64)).astype(np.float32), np.float32(0)).astype(np.float64)


def regime(y1, layers, tail):
    """What regime a case reaches, from the exact (float64) layer-1 output alone: per 16-row tile, whether
    y1 is all zero (dead), whether it has an all-zero row beside a live one (mixed), and the looseness of
    layer 3's scale = bound_exp3's bound / the tile's real max of y2 (inf on a tile whose y2 is all zero)."""
    y1 = np.asarray(y1, np.float64)
    t = y1.reshape(y1.shape[0] // TILE, TILE, -1)
    rowmax = t.max(axis=2)
    dead = rowmax.max(axis=1) == 0
    mixed = (rowmax.min(axis=1) == 0) & ~dead
    e2 = exp_of(t.max(axis=(1, 2)).astype(np.float32))
    y2 = np.maximum(y1 @ np.asarray(layers[1][0], np.float64) + np.asarray(layers[1][1], np.float64), 0.0)
    m2 = y2.reshape(len(t), -1).max(axis=1)
    with np.errstate(divide="ignore"):
        loose = bound_value(tail, e2).astype(np.float64) / m2
    return {"dead": dead, "mixed": mixed, "loose": loose, "zero_frac": float((y1 == 0).mean())}


# ---------------------------------------------------------------------------------- hard cases
def _family(name):
    for base in ("bn_spread", "loose_bound"):
        if name.startswith(base) and name != base:
            return base, int(name[len(base):])
    return name, None


def weight_family(name, widths, cin, seed):
    """[(W (cin, c1), b), (W (c1, c2), b), (W (c2, c3), b)] float32 of the named family (module FAMILIES;
    "bn_spread<s>" and "loose_bound<k>" carry their parameter: a 2^s channel spread, a 2^k factor).

    fresh        init_weights' distribution, U(+-1/sqrt(cin)) for W and b: the regression anchor
    bn_spread s  layers 1 and 2: output channel c times g_c = 2^U(-s/2, s/2), 1/g_c folded into the next
                 layer's row c — the function is unchanged, per-channel weight scales spread over 2^s
    sparse       b1 and b2 negative: most ReLU outputs are zero, and a row with no input gives an all-zero y1
    loose_bound  W1's columns in equal pairs and W2's rows in pairs (w, -w + small): colsum(W2) far above
                 any y2; b2[0] = -2^k: max |b2|, hence layer 3's scale, 2^k above the data
    outlier_row  fresh (xyz levels: b1 = 0, so y1 is as spread as the offsets); the inputs carry the outlier
    tiny / huge  fresh with the biases times 2^-30 / 2^30 (the inputs are scaled alike)"""
    base, par = _family(name)
    rng = np.random.default_rng([seed, cin, *widths])
    layers = []
    for k, c in zip([cin] + list(widths[:-1]), widths):
        bd = 1.0 / np.sqrt(k)
        layers.append([rng.uniform(-bd, bd, (k, c)), rng.uniform(-bd, bd, c)])
    if base == "bn_spread":
        for j in (0, 1):
            g = np.exp2(rng.uniform(-par / 2, par / 2, widths[j]))
            if par:
                g[:2] = np.exp2([-par / 2, par / 2])  # the stated spread is reached, not only approached
            layers[j][0] *= g[None, :]
            layers[j][1] *= g
            layers[j + 1][0] /= g[:, None]
    elif base == "sparse":
        layers[0][1] = -np.abs(layers[0][1]) * (0.06 if cin == 3 else 1.0) - 1e-3
        layers[1][1] = -np.abs(layers[1][1]) * 0.5 - 1e-3
    elif base == "loose_bound":
        W1, b1 = layers[0]
        W1[:, 1::2] = W1[:, 0::2]
        b1[1::2] = b1[0::2]
        W2 = layers[1][0]
        W2[1::2] = -W2[0::2] + 0.125 * W2[1::2]
        layers[1][1][0] = -(2.0 ** par)
    elif base == "outlier_row":
        if cin == 3:
            layers[0][1][:] = 0.0
    elif base in ("tiny", "huge"):
        for lay in layers:
            lay[1] *= 2.0 ** (-30 if base == "tiny" else 30)
    elif base != "fresh":
        raise ValueError(f"unknown family {name}")
    return [(W.astype(np.float32), b.astype(np.float32)) for W, b in layers]


def input_family(name, x, cfeat, seed):
    """(x', f', radius factor) of the named family from frames x (B, N, 3) float32 in the unit cube:
    f' (B, N, cfeat) = |N(0, 1)| features (None for cfeat = 0).

    sparse       points 0 .. PLANT-1 are copies of point 0 with zero features: a centre among them has only
                 dead rows; points PLANT .. PLANT+15 keep their place and lose their features
    outlier_row  every 23rd point's features times 2^12; and 12 points at 2^-12 of the unit around each of
                 the first 8 ordinary centres (xyz levels: offsets 2^-12 of their tile-mates')
    tiny / huge  x, f and the radius times 2^-30 / 2^30 (exact: the neighbourhoods do not change)"""
    base, _ = _family(name)
    rng = np.random.default_rng([seed, 77, cfeat])
    x = np.array(x, dtype=np.float32)
    B, N, _3 = x.shape
    f = np.abs(rng.standard_normal((B, N, cfeat))).astype(np.float32) if cfeat else None
    scale = 1.0
    if base == "sparse":
        x[:, :PLANT] = x[:, :1]
        if f is not None:
            f[:, :PLANT + 16] = 0.0
    elif base == "outlier_row":
        for i in range(8):
            lo = 300 + 12 * i
            x[:, lo:lo + 12] = x[:, PLANT + i][:, None] + (rng.uniform(-1, 1, (B, 12, 3)) * 2.0 ** -12).astype(np.float32)
        if f is not None:
            f[:, ::23] *= np.float32(2.0 ** 12)
    elif base in ("tiny", "huge"):
        scale = 2.0 ** (-30 if base == "tiny" else 30)
        x *= np.float32(scale)
        if f is not None:
            f *= np.float32(scale)
    return x, f, scale


def build_case(shape, family, seed=0, B=2, N=1024, M=37):
    """One single-kernel case: frames, features, centres (points C0 .. C0 + M - 1), the oracle's ball-query
    indices and the family's weights for a fused shape."""
    from oracle import tier_n
    from lidar_ai_recommendation_software_amd.synthetic import unit_frames
    xyz_level, c1, c2, c3, ns = shape
    cfeat = 0 if xyz_level else CFEAT
    x, f, scale = input_family(family, unit_frames(B, N, 100 + seed), cfeat, seed)
    r = float(np.float32(RADII[shape] * scale))
    c = np.ascontiguousarray(x[:, C0:C0 + M])
    return {"shape": shape, "family": family, "x": np.ascontiguousarray(x), "f": f, "c": c, "r": r, "ns": ns,
            "widths": [c1, c2, c3], "cfeat": cfeat, "xyz_level": xyz_level, "scale": scale,
            "gi": tier_n.ball_query(x, c, r, ns), "layers": weight_family(family, [c1, c2, c3], 3 + cfeat, seed)}


def grouped(case, b):
    """Frame b's grouped rows [x_k - c, f_k] (M * ns, 3 + cfeat) float32, as the oracle forms them."""
    from oracle import tier_n
    return tier_n.group(case["x"][b], None if case["f"] is None else case["f"][b], case["c"][b], case["gi"][b])


def exact_forward(y1_pre, layers, group):
    """Exact (float64) layers 2-3 + max-pool of an exact layer-1 pre-activation."""
    h = np.maximum(np.asarray(y1_pre, np.float64), 0.0)
    for W, b in layers[1:]:
        h = np.maximum(h @ np.asarray(W, np.float64) + np.asarray(b, np.float64), 0.0)
    return h.reshape(-1, group, h.shape[1]).max(axis=1)


def feat_close_ok(got, want, rtol=1e-4, rel_floor=1e-2):
    """Whether `got` meets the project's strict feat_close against `want` (tests/test_gpu_tier_n.py): every
    element within rtol |want| + rtol RMS and a pure relative error <= rtol on every element with
    |want| >= rel_floor RMS.  Returns (ok, worst pure relative error)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rms = np.sqrt(np.mean(want ** 2)) + 1e-30
    err = np.abs(got - want)
    big = np.abs(want) >= rel_floor * rms
    worst = float((err[big] / np.abs(want[big])).max()) if big.any() else 0.0
    return bool((err <= rtol * np.abs(want) + rtol * rms).all() and worst <= rtol), worst


def host_layer1(case, b):
    """Frame b's layer-1 input without a GPU, as x3_forward_bound takes it: the grouped offsets of an xyz
    level; for a feature level (P gathered per grouped row, Q per centre) with P = [x, f] W1 + b1 per point
    and Q = c W1_xyz computed in float64 and rounded once to float32 (a stand-in for the GEMMs' output).
    Returns (rows_or_PQ, l1)."""
    if case["xyz_level"]:
        return grouped(case, b), "xyz"
    W1, b1 = (np.asarray(a, np.float64) for a in case["layers"][0])
    pts = np.concatenate([case["x"][b], case["f"][b]], axis=1).astype(np.float64)
    P = (pts @ W1 + b1).astype(np.float32)
    Q = (case["c"][b].astype(np.float64) @ W1[:3]).astype(np.float32)
    return (P[case["gi"][b].reshape(-1)], Q), "pre"


def layer1_exact(rows_or_PQ, layers, group, l1):
    """The exact (float64) layer-1 output after ReLU, (R, c1)."""
    return np.maximum(_layer1(rows_or_PQ, layers[0], group, l1, lambda k: k + 4)[0], 0.0)


def emulation_meets_contract(y1, layers, group, tail):
    """Whether h3.hpp's documented arithmetic (emulate_x3 on the float32 layer-1 output y1) meets the strict
    1e-4 feat_close against the exact layers 2-3 of the same y1: decides which cases also assert feat_close
    on the GPU.  Returns (ok, worst pure relative error)."""
    y1 = np.ascontiguousarray(y1, dtype=np.float32)
    return feat_close_ok(emulate_x3(y1, layers, group, tail), exact_forward(y1, layers, group))
