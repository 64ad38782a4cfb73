"""CPU restatement of the replenishment stage of Tracker::track_features (reference src/Tracker.cpp:127-146) and of the
ORB extractor's detector (features/OrbFeatureExtractor.cpp:5-27, cv::GFTTDetector::create(3000, 0.005, 5)): numpy.
Test infrastructure only — the product package never imports it.

This is cv::goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask, blockSize = 3, gradientSize = 3,
useHarris = false) as OpenCV 4.x implements it, restated with ONE deliberate difference (the KLT precedent,
tests/klt_ref.py): the structure-tensor sums are exact integers, where OpenCV scales dx, dy by 1 / 3060 inside an f32
Sobel and box-sums in f32.  Every later operation is the f32 / f64 operation OpenCV performs, in the same order, so
csrc/gftt.hip (built with -ffp-contract=off, correctly rounded sqrtf) reproduces this file bit for bit.

  derivatives   Sobel 3x3 on the u8 image, reflect-101:  dx = [1 2 1]^T (x) [-1 0 1], dy its transpose (|d| <= 1020)
  tensor        Sxx = sum dx^2, Sxy = sum dx dy, Syy = sum dy^2 over the 3x3 block; the box sum reflects the TENSOR
                image (reflect-101): the tensor at x = -1 is the tensor at x = 1 (each sum < 9 * 1020^2 < 2^24: exact f32)
  eig           calcMinEigenVal in f32, this order:
                  a = f32(Sxx) * 0.5f;  b = f32(Sxy);  c = f32(Syy) * 0.5f
                  u = a - c;  s = u * u + b * b  (two products, then the sum);  r = sqrtf(s)
                  eig = ((a + c) - r) * EIG_SCALE,  EIG_SCALE = f32(1 / 3060^2)  (OpenCV's (1 / 3060)^2 scale of dx, dy)
  threshold     maxVal = max eig where mask != 0 (minMaxLoc with mask; 0 when the mask is empty),
                thr = f32(f64(maxVal) * quality);  eig = eig > thr ? eig : 0  (THRESH_TOZERO)
  candidates    tmp = dilate(eig, 3x3), pixels outside the image not counted; candidate where 1 <= x <= W-2,
                1 <= y <= H-2, eig != 0, eig == tmp, mask != 0
  order         eig descending, ties: larger raster offset y * W + x first (4.x greaterThanPtr on addresses)
  min distance  greedy walk: accept unless an accepted corner lies at dx^2 + dy^2 < minDistance^2; stop at maxCorners;
                minDistance < 1: no filter, only the cap.  (OpenCV's cell grid at cell = cvRound(minDistance) is this
                rule: select_grid transcribes it literally; select_rounds is the parallel form the device runs.)
Around it:
  border        runByImageBorder(31) of ORB's compute: keep 31 <= x < W-31 and 31 <= y < H-31, after the cap
  mask          the static mask with cv::circle(mask, (cvRound(x), cvRound(y)), r, 0, FILLED) at every excluded point:
                drawing.cpp's integer midpoint loop (Circle, LINE_8, fill), clipped to the image; cvRound = half to even
  budget        the first max(0, max_total - n_excluded) of what is left (max_total < 0: no budget)
"""
import numpy as np

from klt_ref import reflect101

F32 = np.float32
EIG_SCALE = F32(1.0 / (3060.0 * 3060.0))
ORB_BORDER = 31


def sobel(img):
    """Sobel 3x3 (dx, dy) of a u8 image, reflect-101: int64 arrays."""
    h, w = img.shape
    s = np.asarray(img, np.int64)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    v = s[ym] + 2 * s + s[yp]                     # vertical smooth
    dx = v[:, xp] - v[:, xm]
    d = s[yp] - s[ym]                             # vertical difference
    dy = d[:, xm] + 2 * d + d[:, xp]
    return dx, dy


def box3(t):
    """3x3 box sum of a tensor image with the tensor image reflected (reflect-101) at the border."""
    h, w = t.shape
    ys = reflect101(np.arange(-1, h + 1), h)
    xs = reflect101(np.arange(-1, w + 1), w)
    p = t[ys][:, xs]
    r = p[:-2] + p[1:-1] + p[2:]
    return r[:, :-2] + r[:, 1:-1] + r[:, 2:]


def tensor(img):
    dx, dy = sobel(img)
    return box3(dx * dx), box3(dx * dy), box3(dy * dy)


def min_eig(sxx, sxy, syy):
    """calcMinEigenVal on exact integer sums, f32 in the documented order, times EIG_SCALE."""
    a = np.asarray(sxx).astype(F32) * F32(0.5)
    b = np.asarray(sxy).astype(F32)
    c = np.asarray(syy).astype(F32) * F32(0.5)
    u = a - c
    s = u * u + b * b
    return ((a + c) - np.sqrt(s)) * EIG_SCALE


def corner_response(img):
    """cornerMinEigenVal(img, 3, 3) restated: eig [h][w] f32."""
    return min_eig(*tensor(np.asarray(img, np.uint8)))


def circle_half_widths(r):
    """drawing.cpp Circle (filled, LINE_8): hw[d] = half width of the union of the spans drawn at rows cy +- d."""
    hw = np.full(r + 1, -1, np.int64)
    err, dx, dy, plus, minus = 0, r, 0, 1, (r << 1) - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)          # rows cy -+ dy: [cx - dx, cx + dx]
        hw[dx] = max(hw[dx], dy)          # rows cy -+ dx: [cx - dy, cx + dy]
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return hw


def stamp_circles(mask, pts, r):
    """cv::circle(mask, Point(cvRound(x), cvRound(y)), r, 0, FILLED) for every point, in place; clipped to the image."""
    h, w = mask.shape
    hw = circle_half_widths(r)
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        cx, cy = int(np.rint(x)), int(np.rint(y))
        for d in range(-r, r + 1):
            yy, k = cy + d, hw[abs(d)]
            if k < 0 or not 0 <= yy < h:
                continue
            x0, x1 = max(cx - k, 0), min(cx + k, w - 1)
            if x0 <= x1:
                mask[yy, x0:x1 + 1] = 0
    return mask


def threshold(eig, mask=None):
    """(thr, max) of goodFeaturesToTrack: maxVal over mask != 0 (0 when empty), thr = f32(maxVal * quality) is applied by
    the caller; returns maxVal as f32."""
    sel = eig if mask is None else eig[np.asarray(mask) != 0]
    return F32(sel.max()) if sel.size else F32(0)


def candidates(eig, mask, quality):
    """-> (thr, offsets of the candidates, ascending)."""
    h, w = eig.shape
    thr = F32(float(threshold(eig, mask)) * float(quality))
    e = np.where(eig > thr, eig, F32(0))
    p = np.full((h + 2, w + 2), -np.inf, np.float32)
    p[1:-1, 1:-1] = e
    tmp = p[1:-1, 1:-1].copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            np.maximum(tmp, p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx], out=tmp)
    c = (e != 0) & (e == tmp)
    if mask is not None:
        c &= np.asarray(mask) != 0
    inner = np.zeros_like(c)
    inner[1:-1, 1:-1] = True
    c &= inner
    return thr, np.flatnonzero(c)


def order(eig, offs):
    """offsets sorted by eig descending, ties by the larger offset first"""
    v = eig.reshape(-1)[offs]
    k = np.lexsort((-offs.astype(np.int64), -v.astype(np.float64)))
    return offs[k]


def select_grid(sorted_offs, width, height, min_distance, max_corners):
    """Literal transcription of goodFeaturesToTrack's minimum-distance walk (OpenCV 4.x, cell grid)."""
    out = []
    if min_distance >= 1:
        cell = int(np.rint(min_distance))
        gw, gh = (width + cell - 1) // cell, (height + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for ofs in sorted_offs:
            y, x = divmod(int(ofs), width)
            good = True
            xc, yc = x // cell, y // cell
            x1, y1, x2, y2 = max(0, xc - 1), max(0, yc - 1), min(gw - 1, xc + 1), min(gh - 1, yc + 1)
            for yy in range(y1, y2 + 1):
                for xx in range(x1, x2 + 1):
                    for (px, py) in grid[yy * gw + xx]:
                        ddx, ddy = F32(x - px), F32(y - py)
                        if float(ddx * ddx + ddy * ddy) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((x, y))
                out.append(int(ofs))
                if max_corners > 0 and len(out) == max_corners:
                    break
    else:
        out = [int(o) for o in (sorted_offs[:max_corners] if max_corners > 0 else sorted_offs)]
    return np.array(out, np.int64)


def disc_offsets(min_distance):
    """(dx, dy) != (0, 0) with dx^2 + dy^2 < min_distance^2"""
    R = int(np.ceil(min_distance))
    return [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
            if (dx or dy) and float(dx * dx + dy * dy) < float(min_distance) * float(min_distance)]


def select_rounds(eig, offs, min_distance, max_corners):
    """The parallel form of the walk (csrc/gftt.hip): rounds over all candidates at once.  A candidate is accepted once
    every higher-priority candidate within the distance is decided and none is accepted, and rejected once one of them
    is accepted; priority is (eig, offset) lexicographically.  -> (accepted offsets in priority order, capped; rounds)."""
    h, w = eig.shape
    so = order(eig, offs)
    if min_distance < 1:
        return so[:max_corners], 0
    rank = np.full(h * w, -1, np.int64)
    rank[so] = len(so) - np.arange(len(so))          # larger = higher priority
    rank = rank.reshape(h, w)
    state = np.zeros((h, w), np.int8)               # 0 none, 1 undecided, 2 accepted, 3 rejected
    state.reshape(-1)[so] = 1
    R = int(np.ceil(min_distance))
    pr = np.pad(rank, R, constant_values=-1)
    rounds = 0
    ys, xs = np.divmod(so, w)
    nb = disc_offsets(min_distance)
    while (state.reshape(-1)[so] == 1).any():
        rounds += 1
        ps = np.pad(state, R)
        und = state.reshape(-1)[so] == 1
        yy, xx, rk = ys[und], xs[und], rank.reshape(-1)[so[und]]
        acc_hi = np.zeros(len(yy), bool)
        und_hi = np.zeros(len(yy), bool)
        for dx, dy in nb:
            qs, qr = ps[yy + R + dy, xx + R + dx], pr[yy + R + dy, xx + R + dx]
            hi = qr > rk
            acc_hi |= hi & (qs == 2)
            und_hi |= hi & (qs == 1)
        new = np.where(acc_hi, 3, np.where(und_hi, 1, 2)).astype(np.int8)
        state[yy, xx] = new
    acc = so[state.reshape(-1)[so] == 2]
    return acc[:max_corners], rounds


def good_features(img, mask=None, max_corners=3000, quality=0.005, min_distance=5.0):
    """goodFeaturesToTrack restated -> (offsets of the corners in output order, eig, thr)."""
    eig = corner_response(img)
    h, w = eig.shape
    thr, offs = candidates(eig, mask, quality)
    sel = select_grid(order(eig, offs), w, h, min_distance, max_corners)
    return sel, eig, thr


def detect_features(img, static_mask=None, exclude_pts=None, radius=5, max_corners=3000, quality=0.005, min_distance=5.0,
                    border=ORB_BORDER, max_total=-1):
    """Tracker.cpp:127-146 with the ORB extractor: replenish mask, GFTT, runByImageBorder, budget.
    -> dict(pts [D][2] f32, response [D] f32, detected D, appended, mask, eig)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    mask = np.full((h, w), 255, np.uint8) if static_mask is None else np.array(static_mask, np.uint8, copy=True)
    n_ex = 0
    if exclude_pts is not None:
        ex = np.asarray(exclude_pts, np.float32).reshape(-1, 2)
        n_ex = len(ex)
        stamp_circles(mask, ex, radius)
    sel, eig, _ = good_features(img, mask, max_corners, quality, min_distance)
    y, x = np.divmod(sel, w)
    keep = (x >= border) & (x < w - border) & (y >= border) & (y < h - border)
    sel = sel[keep]
    y, x = np.divmod(sel, w)
    pts = np.stack([x, y], 1).astype(np.float32)
    resp = eig.reshape(-1)[sel]
    d = len(sel)
    budget = d if max_total < 0 else max(0, max_total - n_ex)
    return dict(pts=pts, response=resp, detected=d, appended=min(d, budget), mask=mask, eig=eig)
