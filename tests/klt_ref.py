"""CPU restatement of the KLT stage (Tracker::track_features, reference src/Tracker.cpp:90-134): numpy, vectorised over
points.  Test infrastructure only — the product package never imports it.

This is Bouguet's pyramidal Lucas-Kanade as OpenCV's calcOpticalFlowPyrLK implements it (buildOpticalFlowPyramid,
calcSharrDeriv, LKTrackerInvoker), restated with ONE deliberate difference: the window sums (A11, A12, A22, b1, b2) are
accumulated exactly in int64 and converted to f32 once, where OpenCV accumulates them in f32.  Every other operation is
the f32 / f64 operation OpenCV performs, in the same order, so csrc/klt.hip (built with -ffp-contract=off) reproduces
this file bit for bit.

  grey           (1868 B + 9617 G + 4899 R + 8192) >> 14                     cv::cvtColor BGR2GRAY, 8-bit path
  pyramid        pyrDown: [1 4 6 4 1]^T [1 4 6 4 1], (s + 128) >> 8, reflect-101, size ((w+1)/2, (h+1)/2); a level is
                 built only while its size exceeds the window in both directions (buildOpticalFlowPyramid's clamp)
  derivatives    Scharr, int16: dx = [3 10 3]^T (x) [-1 0 1], dy its transpose, reflect-101 inside the level
  padding        image levels reflect-101 by `win`, derivative images zeros by `win`
  LK             per level from the top: W_BITS = 14 bilinear weights, template DESCALE(., 9) (x32) and DESCALE(., 14),
                 minEig / det gate, at most max_iter Newton steps, |delta|^2 <= eps^2 stop, oscillation back-off
"""
import numpy as np

W_BITS = 14
FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
F32 = np.float32


def to_grey(img):
    """1-channel passes through; 3-channel is BGR (Tracker.cpp:24-32)."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img
    b, g, r = (img[..., c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), vectorised (any p, n >= 1)."""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p, p)
        p = np.where(hi, 2 * (n - 1) - p, p)


def pyr_down(img):
    h, w = img.shape
    H, W = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int64)
    rows = reflect101(2 * np.arange(H)[:, None] + np.arange(-2, 3)[None, :], h)     # [H][5]
    cols = reflect101(2 * np.arange(W)[:, None] + np.arange(-2, 3)[None, :], w)     # [W][5]
    src = img.astype(np.int64)
    t = np.einsum("yk,ykx->yx", np.broadcast_to(k, rows.shape), src[rows])           # vertical pass  [H][w]
    s = np.einsum("xk,yxk->yx", np.broadcast_to(k, cols.shape), t[:, cols])          # horizontal pass [H][W]
    return ((s + 128) >> 8).astype(np.uint8)


def scharr(img):
    """calcSharrDeriv: (dx, dy) int16, reflect-101 inside the image."""
    h, w = img.shape
    src = img.astype(np.int64)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    t0 = (src[ym] + src[yp]) * 3 + src * 10          # vertical smooth
    t1 = src[yp] - src[ym]                           # vertical difference
    dx = t0[:, xp] - t0[:, xm]
    dy = (t1[:, xp] + t1[:, xm]) * 3 + t1 * 10
    return dx.astype(np.int16), dy.astype(np.int16)


def num_levels(width, height, win, max_level):
    """Highest level buildOpticalFlowPyramid builds: level l + 1 exists only if its size exceeds `win` both ways."""
    w, h = width, height
    for lvl in range(max_level + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            return lvl
    return max_level


def build_pyramid(img, win=21, max_level=4):
    """List of levels: dict(w, h, img = interior u8 [h][w], pad = reflect-101 padded u8 [h+2win][w+2win],
    dx / dy = zero-padded int16 [h+2win][w+2win])."""
    g = to_grey(img)
    top = num_levels(g.shape[1], g.shape[0], win, max_level)
    out = []
    for lvl in range(top + 1):
        if lvl:
            g = pyr_down(g)
        h, w = g.shape
        pad = g[reflect101(np.arange(-win, h + win), h)][:, reflect101(np.arange(-win, w + win), w)]
        dx, dy = scharr(g)
        px = np.zeros((h + 2 * win, w + 2 * win), np.int16)
        py = np.zeros_like(px)
        px[win:win + h, win:win + w] = dx
        py[win:win + h, win:win + w] = dy
        out.append(dict(w=w, h=h, img=g, pad=pad, dx=px, dy=py))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    """f32 a, b -> int64 iw00, iw01, iw10, iw11 (cvRound = round half to even)."""
    one, s = F32(1), F32(1 << W_BITS)
    iw00 = np.rint((one - a) * (one - b) * s).astype(np.int64)
    iw01 = np.rint(a * (one - b) * s).astype(np.int64)
    iw10 = np.rint((one - a) * b * s).astype(np.int64)
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _gather(buf, ix, iy, win, w):
    """Bilinear corner values of the win x win window at floored origins (ix, iy) (level coordinates) in a buffer padded
    by `w`: 4 arrays [n][win*win] int64."""
    r = np.arange(win)
    X = (ix[:, None] + w + np.tile(r, win)[None, :])
    Y = (iy[:, None] + w + np.repeat(r, win)[None, :])
    b = buf.astype(np.int64)
    return b[Y, X], b[Y, X + 1], b[Y + 1, X], b[Y + 1, X + 1]


def _in_window(fx, fy, cols, rows, win):
    """floored origin inside [-win, cols) x [-win, rows); NaN fails"""
    return (fx >= -win) & (fx < cols) & (fy >= -win) & (fy < rows)


def _template(I, prev, win, pad):
    """The window of level I at the level positions `prev` (f32 [n][2]): -> (ok = the window test, idx = its passing
    points, and for those the template tI, tX, tY [m][win*win], the f32 matrix A11, A12, A22, its determinant D and
    minimum eigenvalue mine [m])."""
    prev = prev - F32((win - 1) * 0.5)
    fx, fy = np.floor(prev[:, 0]), np.floor(prev[:, 1])
    ok = _in_window(fx, fy, I["w"], I["h"], win)
    idx = np.nonzero(ok)[0]
    ix, iy = fx[idx].astype(np.int64), fy[idx].astype(np.int64)
    a, b = prev[idx, 0] - fx[idx], prev[idx, 1] - fy[idx]
    w00, w01, w10, w11 = (w[:, None] for w in _weights(a, b))
    c = _gather(I["pad"], ix, iy, win, pad)
    tI = _descale(c[0] * w00 + c[1] * w01 + c[2] * w10 + c[3] * w11, W_BITS - 5)
    c = _gather(I["dx"], ix, iy, win, pad)
    tX = _descale(c[0] * w00 + c[1] * w01 + c[2] * w10 + c[3] * w11, W_BITS)
    c = _gather(I["dy"], ix, iy, win, pad)
    tY = _descale(c[0] * w00 + c[1] * w01 + c[2] * w10 + c[3] * w11, W_BITS)
    A11 = (tX * tX).sum(1).astype(np.float32) * FLT_SCALE
    A12 = (tX * tY).sum(1).astype(np.float32) * FLT_SCALE
    A22 = (tY * tY).sum(1).astype(np.float32) * FLT_SCALE
    D = A11 * A22 - A12 * A12
    d = A11 - A22
    mine = (A22 + A11 - np.sqrt(d * d + F32(4) * A12 * A12)) / F32(2 * win * win)
    return ok, idx, tI, tX, tY, A11, A12, A22, D, mine


def min_eigenvalues(pyr, pts, win=21, level=0):
    """The minEig that lk compares with min_eig at `level` for each point of `pts` (level-0 coordinates): f32 [n], NaN
    where the window test fails there."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    pad = pyr[0]["pad"].shape[0] - pyr[0]["h"] >> 1
    ok, idx, *_, mine = _template(pyr[level], pts * F32(1.0 / (1 << level)), win, pad)
    out = np.full(len(pts), np.nan, np.float32)
    out[idx] = mine
    return out


def lk(prev_pyr, next_pyr, pts, guess=None, win=21, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4):
    """calcOpticalFlowPyrLK(prev, next, pts, guess) -> (next_pts [n][2] f32, status [n] u8)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    top = min(max_level, len(prev_pyr) - 1, len(next_pyr) - 1, num_levels(prev_pyr[0]["w"], prev_pyr[0]["h"], win, max_level))
    pad = prev_pyr[0]["pad"].shape[0] - prev_pyr[0]["h"] >> 1
    assert win <= pad
    status = np.ones(n, np.uint8)
    nxt = np.zeros((n, 2), np.float32)
    half = F32((win - 1) * 0.5)
    eps2 = float(eps) * float(eps)
    for lvl in range(top, -1, -1):
        I, J = prev_pyr[lvl], next_pyr[lvl]
        prev = pts * F32(1.0 / (1 << lvl))
        if lvl == top:
            nxt = prev.copy() if guess is None else np.asarray(guess, np.float32).reshape(-1, 2) * F32(1.0 / (1 << lvl))
        else:
            nxt = nxt * F32(2)
        ok, idx, tI, tX, tY, A11, A12, A22, D, mine = _template(I, prev, win, pad)
        if lvl == 0:
            status[~ok] = 0
        if len(idx) == 0:
            continue
        bad = (mine.astype(np.float64) < min_eig) | (D < FLT_EPSILON)
        if lvl == 0:
            status[idx[bad]] = 0
        keep = ~bad
        idx, tI, tX, tY = idx[keep], tI[keep], tX[keep], tY[keep]
        A11, A12, A22 = A11[keep], A12[keep], A22[keep]
        Dinv = F32(1) / D[keep]
        p = nxt[idx] - half
        pd = np.zeros((len(idx), 2), np.float32)
        act = np.arange(len(idx))
        for j in range(max_iter):
            if len(act) == 0:
                break
            q = p[act]
            gx, gy = np.floor(q[:, 0]), np.floor(q[:, 1])
            inw = _in_window(gx, gy, J["w"], J["h"], win)
            if lvl == 0:
                status[idx[act[~inw]]] = 0
            act, q, gx, gy = act[inw], q[inw], gx[inw], gy[inw]
            if len(act) == 0:
                break
            w00, w01, w10, w11 = (w[:, None] for w in _weights(q[:, 0] - gx, q[:, 1] - gy))
            c = _gather(J["pad"], gx.astype(np.int64), gy.astype(np.int64), win, pad)
            diff = _descale(c[0] * w00 + c[1] * w01 + c[2] * w10 + c[3] * w11, W_BITS - 5) - tI[act]
            b1 = (diff * tX[act]).sum(1).astype(np.float32) * FLT_SCALE
            b2 = (diff * tY[act]).sum(1).astype(np.float32) * FLT_SCALE
            a11, a12, a22, di = A11[act], A12[act], A22[act], Dinv[act]
            dx = (a12 * b2 - a22 * b1) * di
            dy = (a12 * b1 - a11 * b2) * di
            q = np.stack([q[:, 0] + dx, q[:, 1] + dy], 1)
            p[act] = q
            out = q + half
            conv = dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64) <= eps2
            osc = ~conv & (j > 0) & (np.abs(dx + pd[act, 0]).astype(np.float64) < 0.01) & \
                (np.abs(dy + pd[act, 1]).astype(np.float64) < 0.01)
            out[osc, 0] -= dx[osc] * F32(0.5)
            out[osc, 1] -= dy[osc] * F32(0.5)
            nxt[idx[act]] = out
            pd[act, 0], pd[act, 1] = dx, dy
            act = act[~(conv | osc)]
    return nxt, status


def fb_filter(prev_pts, next_pts, back_pts, ok_f, ok_b, width, height, mask=None, fb_max=1.0):
    """Tracker.cpp:115-126 -> ascending kept indices."""
    prev_pts = np.asarray(prev_pts, np.float32).reshape(-1, 2)
    d = prev_pts - back_pts                                          # Point2f difference (f32)
    nrm = np.sqrt(d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2)   # cv::norm(Point2f), f64
    keep = (ok_f != 0) & (ok_b != 0) & ~(nrm > float(np.float32(fb_max)))
    rx, ry = np.rint(next_pts[:, 0]), np.rint(next_pts[:, 1])     # cvRound: half to even
    inside = (rx >= 0) & (ry >= 0) & (rx < width) & (ry < height)
    keep &= inside
    if mask is not None:
        ii = np.nonzero(keep)[0]
        keep[ii] = np.asarray(mask)[ry[ii].astype(np.int64), rx[ii].astype(np.int64)] != 0
    return np.nonzero(keep)[0].astype(np.int32)


def track_features(prev_pyr, next_pyr, pts, mask=None, fb_max=1.0, win=21, max_level=4, max_iter=30, eps=0.01,
                   min_eig=1e-4):
    """Tracker::track_features steps 2-4 -> dict(index = kept indices, pts = their new positions, and the raw passes)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    nf, sf = lk(prev_pyr, next_pyr, pts, None, win, max_level, max_iter, eps, min_eig)
    nb, sb = lk(next_pyr, prev_pyr, nf, None, win, max_level, max_iter, eps, min_eig)
    idx = fb_filter(pts, nf, nb, sf, sb, next_pyr[0]["w"], next_pyr[0]["h"], mask, fb_max)
    return dict(index=idx, pts=nf[idx], next=nf, status_f=sf, back=nb, status_b=sb)
