"""numpy model of the integrated loudness of include/waa_hip_device.h (waa_output_loudness & co.), written from the
definitions there and from nothing else: the serial recurrence of the K-weighting, vectorised over rows, in f64 or — the reference
of the tests — in np.longdouble; the sub-block energies; blocks and gates; and a first-order bound on what f64 arithmetic, serial or
split over sub-blocks as the device splits it, may differ from the exact value by."""
import math

import numpy as np

U = 2.0 ** -53
NEG_INF = -math.inf


def hop(sr):
    return int(math.floor(sr / 10.0 + 0.5))


def coefficients(sr):
    """((b0, b1, b2, a1, a2) of the shelf, (1, -2, 1, a1, a2) of the high-pass): Python floats, f64 arithmetic"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return shelf, (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)


def entering(x):
    """the samples as they enter, f64: e == 255 and e == 0 as +0.0, every other sample as (double)x"""
    x = np.ascontiguousarray(x, np.float32)
    e = (x.view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(23)
    return np.where((e >= 1) & (e <= 254), x.astype(np.float64), 0.0)


def _run(xt, state, co, dtype, track):
    """the cascade over xt[frames, lanes] from state (a list of four arrays [lanes], replaced by the end state).  Returns
    (z, e1, e2): z[lanes], the ascending sum of w^2 over the frames given; with `track`, e1 / e2[frames, lanes], the magnitudes that
    the roundings of the shelf / of the high-pass are relative to (see bound), else None"""
    (b0, b1, b2, a1, a2), (_, _, _, c1, c2) = [[dtype(v) for v in s] for s in co]
    p1, p2, q1, q2 = state
    z = np.zeros(xt.shape[1], dtype)
    two = dtype(-2.0)
    e1 = e2 = None
    if track:
        e1, e2 = np.empty(xt.shape, np.float64), np.empty(xt.shape, np.float64)
        kx, kv, kw = abs(float(b0)) + 2 * abs(float(b1)) + abs(float(b2)), 1 + 2 * abs(float(a1)) + abs(float(a2)), 1 + 2 * abs(float(c1)) + abs(float(c2))
    for n in range(xt.shape[0]):
        x = xt[n]
        v = b0 * x + p1
        p1 = (b1 * x - a1 * v) + p2
        p2 = b2 * x - a2 * v
        w = v + q1
        q1 = (two * v - c1 * w) + q2
        q2 = v - c2 * w
        z = z + w * w
        if track:
            av, aw = np.abs(v), np.abs(w)
            e1[n] = kx * np.abs(x) + kv * av + np.abs(p1) + np.abs(p2)
            e2[n] = kw * aw + 2.0 * av + np.abs(q1) + np.abs(q2)
    state[0], state[1], state[2], state[3] = p1, p2, q1, q2
    return z, e1, e2


def series(x, sr, dtype=np.float64, track=False):
    """z[..., n_sub] of x[..., L] (f32) in `dtype` arithmetic, the serial recurrence from zero state.  track: also a dict with
    `start` [n_sub, 4, rows], the state in front of every sub-block, and e1, e2 [rows, n_sub * h] (see _run)."""
    x = np.asarray(x, np.float32)
    lead, L = x.shape[:-1], x.shape[-1]
    h = hop(sr)
    n_sub = L // h
    rows = int(np.prod(lead, dtype=np.int64))
    xs = entering(x).reshape(rows, L)[:, :n_sub * h].astype(dtype)
    xt = np.ascontiguousarray(xs.T)  # [frames, rows]
    co = coefficients(sr)
    state = [np.zeros(rows, dtype) for _ in range(4)]
    z = np.zeros((n_sub, rows), dtype)
    start = np.zeros((n_sub, 4, rows), dtype)
    e1 = np.zeros((n_sub * h, rows)) if track else None
    e2 = np.zeros((n_sub * h, rows)) if track else None
    for j in range(n_sub):
        start[j] = state
        z[j], a, b = _run(xt[j * h:(j + 1) * h], state, co, dtype, track)
        if track:
            e1[j * h:(j + 1) * h], e2[j * h:(j + 1) * h] = a, b
    out = np.ascontiguousarray(z.T).reshape(lead + (n_sub,))
    if not track:
        return out
    return out, dict(start=start, e1=np.ascontiguousarray(e1.T), e2=np.ascontiguousarray(e2.T), h=h, n_sub=n_sub, rows=rows)


def transition(sr, dtype=np.float64):
    """M^h [4, 4]: the state after h frames of zero input from each unit state, by the recurrence itself"""
    h = hop(sr)
    state = [np.zeros(4, dtype) for _ in range(4)]
    for c in range(4):
        state[c][c] = dtype(1.0)
    _run(np.zeros((h, 4), dtype), state, coefficients(sr), dtype, False)
    return np.stack(state)  # [r, c]


# ---- blocks and gates -------------------------------------------------------------------------------------------------------------
def default_weights(n_ch):
    return {6: [1.0, 1.0, 1.0, 0.0, 1.41, 1.41], 4: [1.0, 1.0, 1.41, 1.41]}.get(n_ch, [1.0] * n_ch)


def lufs(p):
    return -0.691 + 10.0 * math.log10(p) if p > 0 else NEG_INF


def window_powers(z, h, weights, n):
    """P of every window of n sub-blocks of one context's z[n_ch, n_sub]: Python floats, ascending sums"""
    z = np.asarray(z, np.float64)
    n_ch, n_sub = z.shape
    out = []
    for k in range(n_sub - n + 1):
        p = 0.0
        for c in range(n_ch):
            s = float(z[c, k])
            for i in range(1, n):
                s = s + float(z[c, k + i])
            p = p + weights[c] * s
        out.append(p / (float(n) * float(h)))
    return out


def gating(z, h, weights=None):
    """the loudness record of one context from z[n_ch, n_sub], as a dict; `l` holds every l_k"""
    z = np.asarray(z, np.float64)
    g = default_weights(z.shape[0]) if weights is None else [float(v) for v in weights]
    p = window_powers(z, h, g, 4)
    l = [lufs(v) for v in p]
    r = dict(integrated=NEG_INF, momentary_max=max(l, default=NEG_INF), short_term_max=NEG_INF, relative_threshold=NEG_INF,
             n_blocks=len(p), n_gated=0, l=l)
    a = [k for k in range(len(p)) if l[k] > -70.0]
    if a:
        s = 0.0
        for k in a:
            s = s + p[k]
        r["relative_threshold"] = lufs(s / float(len(a))) - 10.0
        b = [k for k in a if l[k] > r["relative_threshold"]]
        r["n_gated"] = len(b)
        if b:
            s = 0.0
            for k in b:
                s = s + p[k]
            r["integrated"] = lufs(s / float(len(b)))
    r["short_term_max"] = max((lufs(v) for v in window_powers(z, h, g, 30)), default=NEG_INF)
    return r


def gate_margin(r):
    """how far the nearest l_k is from a threshold it is compared with, in LU (inf when nothing is near any)"""
    d = [abs(v + 70.0) for v in r["l"] if v > NEG_INF]
    if r["relative_threshold"] > NEG_INF:
        d += [abs(v - r["relative_threshold"]) for v in r["l"] if v > -70.0]
    return min(d, default=math.inf)


# ---- the bound --------------------------------------------------------------------------------------------------------------------
def _impulse(a1, a2, n, b=None):
    """n taps of 1 / A(z), or of B(z) / A(z)"""
    y = np.zeros(n)
    y1 = y2 = 0.0
    for k in range(n):
        v = (1.0 if k == 0 else 0.0) - a1 * y1 - a2 * y2
        y[k] = v
        y2, y1 = y1, v
    if b is not None:
        y = np.convolve(y, np.asarray(b))[:n]
    return y


def site_responses(sr, n_taps):
    """|impulse response| from a rounding site to w: g12 for every site of the shelf (a value added into v, p1 or p2 passes
    1 / A1 — with a delay that no norm sees — and then the whole high-pass), g2 for every site of the high-pass (1 / A2)"""
    (_, _, _, a1, a2), (b0, b1, b2, c1, c2) = coefficients(sr)
    g1 = _impulse(a1, a2, n_taps)
    hp = _impulse(c1, c2, n_taps, (b0, b1, b2))
    return np.abs(np.convolve(g1, hp)[:n_taps]), np.abs(_impulse(c1, c2, n_taps))


SEGMENTS = 8   # the magnitudes are tracked per h // SEGMENTS frames


def bound(x, sr):
    """(z, bz): the np.longdouble z[..., n_sub] and a first-order bound on |z_f64 - z| for f64 arithmetic of the definition, serial
    or split as the device splits it.  The derivation (u = 2^-53):

    Rounding sites.  Every f64 operation of a frame errs by at most u |its result|.  The shelf's nine results are bounded by
      e1 = (|b0| + 2 |b1| + |b2|) |x| + (1 + 2 |a1| + |a2|) |v| + |p1| + |p2|
    (b1 x - a1 v by the sum of its parts) and the high-pass's, whose 1 * v and -2 * v are exact, by
      e2 = (1 + 2 |c1| + |c2|) |w| + 2 |v| + |q1| + |q2|.
    An error added to v, p1 or p2 reaches w through g12 = (1 / A1) * H2, one added to w, q1 or q2 through g2 = 1 / A2, so
      |dw[n]| <= u sum_k (|g12[k]| e1[n - k] + |g2[k]| e2[n - k]).                                                      (1)
    The cascade is linear: the split scheme's zero-state pass, chain and exact pass compute the same w, and a rounding made at
    frame i reaches w[n] through the same g whether the pass that made it was the exact pass (i in n's sub-block) or the zero-state
    pass (i before it) — each frame's roundings count ONCE.  The zero-state pass works on the serial values less the zero-input
    answer to its sub-block's start state, so its magnitudes are at most serial + |that answer|: e1, e2 are evaluated as that sum,
    frame by frame (the answer is computed from the start states).  (1) is evaluated per segment of s = h // 8 frames: a tap k lands
    floor(k / s) or floor(k / s) + 1 segments back, so with G_d = sum of |g[k]| over floor(k / s) = d and
    mm[q] = max(m[q], m[q - 1]) of the segment maxima m,  |dw| in segment q <= u sum_d G_d mm[q - d]; taps past 3 h meet the
    running maximum.
    The chain adds, at every boundary, the roundings of S' = M S + E (eight operations per element, each at most
    u (2 sum_c |M_rc| |S_c| + |S'_r|)) and the error of M itself (|M_f64 - M_longdouble|, measured) times |S|; such a state error
    reaches w through the same responses, once per boundary: sum_b |g[n - b h]| d_b <= ||g||_1 max_b d_b.
    From w to z: |dz| <= 2 sqrt(h z) |dw|_max + h |dw|_max^2, plus the (h + 2) u z of squaring and adding h terms.  The reference
    itself is longdouble arithmetic of the same form: 2^-11 of all this, covered by the factor 1 + 2^-9."""
    z, t = series(x, sr, np.longdouble, track=True)
    h, n_sub, rows = t["h"], t["n_sub"], t["rows"]
    lead = z.shape[:-1]
    if n_sub == 0:
        return z, np.zeros(z.shape)
    co = coefficients(sr)
    # the zero-input answer to every sub-block's start state, all sub-blocks at once
    state = [np.ascontiguousarray(t["start"][:, r, :]).reshape(-1).astype(np.float64) for r in range(4)]
    _, f1, f2 = _run(np.zeros((h, n_sub * rows)), state, co, np.float64, True)  # [h, n_sub * rows]
    f1 = f1.reshape(h, n_sub, rows).transpose(2, 1, 0).reshape(rows, n_sub * h)
    f2 = f2.reshape(h, n_sub, rows).transpose(2, 1, 0).reshape(rows, n_sub * h)
    s = max(h // SEGMENTS, 1)
    frames = n_sub * h
    n_seg = -(-frames // s)

    def seg_max(e):
        pad = np.zeros((rows, n_seg * s))
        pad[:, :frames] = e
        return pad.reshape(rows, n_seg, s).max(axis=2)

    n_taps = 3 * h
    dw = np.zeros((rows, n_seg))
    for g, m in zip(site_responses(sr, n_taps), (seg_max(t["e1"] + f1), seg_max(t["e2"] + f2))):
        mm = np.maximum(m, np.concatenate([np.zeros((rows, 1)), m[:, :-1]], axis=1))
        run = np.maximum.accumulate(m, axis=1)
        n_d = -(-n_taps // s)
        G = np.array([g[d * s:(d + 1) * s].sum() for d in range(n_d)])
        for d in range(n_d):
            if d >= n_seg:
                break
            dw[:, d:] += U * G[d] * mm[:, :n_seg - d]
        # the taps past n_taps: both responses shrink by e^-24 per h from their peak on (the poles scale with the rate), so the rest
        # is within a few percent of the last segment's sum: n_d times that sum covers it many times over
        dw += U * run * (G[-1] * n_d)
    # the chain
    M64, Mld = transition(sr), transition(sr, np.longdouble)
    dM = np.abs((M64.astype(np.longdouble) - Mld).astype(np.float64))
    aM = np.abs(M64)
    S = np.abs(t["start"].astype(np.float64))  # [n_sub, 4, rows]
    g12, g2 = site_responses(sr, n_taps)
    norm = np.array([g12.sum(), g12.sum(), g2.sum(), g2.sum()]) * 1.001
    chain = np.zeros((n_sub, rows))
    worst = np.zeros((4, rows))
    for j in range(1, n_sub):
        for r in range(4):
            d = 8 * U * (2 * (aM[r][:, None] * S[j - 1]).sum(axis=0) + S[j, r]) + (dM[r][:, None] * S[j - 1]).sum(axis=0)
            worst[r] = np.maximum(worst[r], d)
        chain[j] = (norm[:, None] * worst).sum(axis=0)
    # per sub-block: the largest |dw| of the segments that meet it
    bw = np.zeros((rows, n_sub))
    for j in range(n_sub):
        q0, q1 = (j * h) // s, ((j + 1) * h - 1) // s
        bw[:, j] = dw[:, q0:q1 + 1].max(axis=1) + chain[j]
    z64 = z.reshape(rows, n_sub).astype(np.float64)
    bz = (2.0 * np.sqrt(h * z64) * bw + h * bw * bw + (h + 2) * U * z64) * (1.0 + 2.0 ** -9)
    return z, bz.reshape(lead + (n_sub,))


def lufs_bound(z, bz, h, weights=None):
    """what a window's loudness may move by when every z moves by at most bz: per window the relative change of P through
    10 log10 (first order, and exactly bounded by -10 log10(1 - r) for r < 1), plus two ulps of the logarithm's result; the largest
    over the windows of 4 and of 30 sub-blocks of one context, in LU"""
    z, bz = np.asarray(z, np.float64), np.asarray(bz, np.float64)
    g = default_weights(z.shape[0]) if weights is None else [float(v) for v in weights]
    worst, count = 0.0, max(z.shape[1] - 3, 0)
    for n in (4, 30):
        p, dp = window_powers(z, h, g, n), window_powers(bz, h, g, n)
        for a, b in zip(p, dp):
            if a > 0:
                r = b / a + (n + 8) * U   # (the sums and the division of P itself)
                worst = max(worst, -10.0 * math.log10(1.0 - r) if r < 1 else math.inf)
    # (a gated mean moves by no more than its most-moved block, relatively; adding `count` of them rounds count times;
    # |l| <= 80 wherever it is compared)
    return worst + count * U * 4.35 + 2 * 2.0 ** -52 * 80.0
