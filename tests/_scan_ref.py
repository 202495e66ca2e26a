"""The scanimate checker: phosphor_dot(), scanimate_modify_raster() and composite_layer() of ffmpeg_scanimate.cpp
(:817-974) restated in NumPy float64, every expression in the tool's order and association.  The accumulator is an
integer sum, + - * / sqrt floor ceil are IEEE operations in NumPy as in C, and the tool's two libm calls go through
math.sin / math.cos (never np.sin / np.cos, whose vector forms are not libm), so the checker is bit-identical to the
tool: tests/test_scan_ref.py holds it against fields recorded from the reference's own lines.

scan_field() is the vectorised form, scan_field_scalar() a plain loop over dots and pixels used to check it."""
import math

import numpy as np

M_PI = math.pi


def effect_of(fieldno):
    """:865-867 in the tool's types (effect is an unsigned int before the % 4)."""
    e = (int(fieldno) // 180) & 0xFFFFFFFF
    ef_field = (int(fieldno) - ((e * 180) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return e % 4, ef_field


def field_of(fieldno):
    return (int(fieldno) & 1) ^ 1


def source_rows(sh, inntsc, field):
    return range(field, sh, 2) if inntsc else range(0, sh, 1)


def dot_radius_of(dh, sh, inntsc):
    r = (float(dh) * (2.05 if inntsc else 1.05)) / sh
    return 1.2 if r < 1.2 else r                                                 # :953 (no effect changes the radius)


def bgra_of(acc, field):
    """:965-971: rows field .. of the frame; row 0 of a field == 1 frame stays as the tool's memset leaves it."""
    g = np.minimum(acc >> 1, 255).astype(np.uint8)
    out = np.empty(acc.shape + (4,), np.uint8)
    out[..., 0] = out[..., 1] = out[..., 2] = g
    out[..., 3] = 255
    out[:field] = 0
    return out


def make_source(sw, sh, seed, lo=0, hi=256):
    """A BGRA source frame of uniform random bytes; some green bytes forced to 0 (a dot that draws nothing) and 255."""
    rs = np.random.RandomState(seed)
    f = rs.randint(lo, hi, size=(sh, sw, 4)).astype(np.uint8)
    f[rs.randint(0, sh, 7), rs.randint(0, sw, 7), 1] = 0
    if hi == 256:
        f[rs.randint(0, sh, 7), rs.randint(0, sw, 7), 1] = 255
    return f


def _dots(src, dw, dh, inntsc, fieldno):
    """Per dot (rows x samples): sx, sy, signal behind the effect and the * sigscalxy; the radius."""
    sh, sw = src.shape[0], src.shape[1]
    field = field_of(fieldno)
    ystep = 2 if inntsc else 1
    w2 = sw << 1
    ys = np.array(list(source_rows(sh, inntsc, field)), dtype=np.int64)
    x = np.arange(w2, dtype=np.float64)[None, :]
    y = ys.astype(np.float64)[:, None]
    sigscalxy = (float(dw) / sw) * (float(dh) / sh) * 0.9                        # :928
    sx = np.broadcast_to(((x * 2) / w2) - 1.0, (len(ys), w2)).copy()             # :931
    sy = ((y * 2) / sh) - 1.0                                                    # :932
    sy = sy + (((x * ystep) / w2) / sh)                                          # :944
    green = src[ys][:, np.arange(w2) >> 1, 1].astype(np.float64)
    signal = green / 255                                                         # :947
    effect, ef_field = effect_of(fieldno)
    if effect == 3:
        ef_t = math.sin((float(ef_field) * M_PI * 2) / (59.94 * 1))
        num = ((ys[:, None] * sw * 2 + np.arange(w2)[None, :]) & 0xFFFFFFFF).astype(np.float64)
        frame_t = num / float(sw * sh * 2)                                       # :949
        arg = frame_t * M_PI * 2 * 6
        s = np.array([math.sin(v) for v in arg.ravel()]).reshape(arg.shape)
        c = np.array([math.cos(v) for v in arg.ravel()]).reshape(arg.shape)
        sx = sx + s * ef_t * 0.1
        sy = sy + c * ef_t * 0.1
    elif effect == 1:
        ef_t = float(ef_field) / (60 * 3)
        sy = sy * (1.0 - (ef_t * 2.0))
        signal = signal * abs(1.0 - (ef_t * 2.0))
    elif effect == 2:
        ef_t = float(ef_field) / (60 * 3)
        sy = sy * (1.0 + (ef_t * 12))
    else:
        ef_t = float(ef_field) / (60 * 3)
        f = (((sy + 1.0) / 2.0) * (1.0 - ef_t)) + ef_t
        sx = sx * f
        signal = signal * f
    signal = signal * sigscalxy                                                  # :954
    return sx, sy, signal, dot_radius_of(dh, sh, inntsc)


def scan_field(src, dw, dh, inntsc, fieldno):
    """composite_layer() for one field.  Returns (acc uint32 [dh, dw], frame uint8 [dh, dw, 4])."""
    sx, sy, signal, r = _dots(src, dw, dh, inntsc, fieldno)
    sx, sy, signal = sx.ravel(), sy.ravel(), signal.ravel()
    signal = np.clip(signal, 0.0, 32.0)                                          # :822-824
    live = signal != 0
    sx, sy, signal = sx[live], sy[live], signal[live]
    x = ((sx + 1.0) * dw) / 2                                                    # :827-830
    y = ((sy + 1.0) * dh) / 2
    signal = signal / r                                                          # :833
    iy0 = np.floor(y - r).astype(np.int64)
    ymax = np.floor(y + r).astype(np.int64)
    xmin = np.floor(x - r).astype(np.int64)
    xmax = np.ceil(x + r).astype(np.int64)
    acc = np.zeros(dh * dw, np.uint32)
    ny = int((ymax - iy0).max()) + 1 if len(x) else 0
    nx = int((xmax - xmin).max()) + 1 if len(x) else 0
    for oy in range(ny):
        iy = iy0 + oy
        rowok = (iy <= ymax) & (iy >= 0) & (iy < dh)
        if not rowok.any():
            continue
        dy = iy.astype(np.float64) - y
        for ox in range(nx):
            ix = xmin + ox
            ok = rowok & (ix <= xmax) & (ix >= 0) & (ix < dw)
            if not ok.any():
                continue
            dx = ix[ok].astype(np.float64) - x[ok]
            dyk = dy[ok]
            fv = signal[ok] * ((r - np.sqrt((dx * dx) + (dyk * dyk))) / r)       # :845
            pos = fv > 0
            v = (fv[pos] * 255).astype(np.int64).astype(np.uint32)              # :847, truncation
            np.add.at(acc, (iy[ok][pos] * dw) + ix[ok][pos], v)
    acc = acc.reshape(dh, dw)
    return acc, bgra_of(acc, field_of(fieldno))


def scan_field_scalar(src, dw, dh, inntsc, fieldno):
    """The same, one dot and one pixel at a time, as the tool's loops run."""
    sh, sw = src.shape[0], src.shape[1]
    field = field_of(fieldno)
    ystep = 2 if inntsc else 1
    w2 = sw << 1
    effect, ef_field = effect_of(fieldno)
    acc = [0] * (dw * dh)
    sigscalxy = (float(dw) / sw) * (float(dh) / sh) * 0.9
    for y in source_rows(sh, inntsc, field):
        for x in range(w2):
            sx = ((float(x) * 2) / w2) - 1.0
            sy = ((float(y) * 2) / sh) - 1.0
            r = (float(dh) * (2.05 if inntsc else 1.05)) / sh
            sy += ((float(x) * ystep) / w2) / sh
            signal = float(src[y, x >> 1, 1]) / 255
            frame_t = float((y * sw * 2 + x) & 0xFFFFFFFF) / (sw * sh * 2)
            if effect == 3:
                ef_t = math.sin((float(ef_field) * M_PI * 2) / (59.94 * 1))
                sx += math.sin(frame_t * M_PI * 2 * 6) * ef_t * 0.1
                sy += math.cos(frame_t * M_PI * 2 * 6) * ef_t * 0.1
            elif effect == 1:
                ef_t = float(ef_field) / (60 * 3)
                sy *= (1.0 - (ef_t * 2.0))
                signal *= abs(1.0 - (ef_t * 2.0))
            elif effect == 2:
                ef_t = float(ef_field) / (60 * 3)
                sy *= (1.0 + (ef_t * 12))
            else:
                ef_t = float(ef_field) / (60 * 3)
                sx *= ((((sy + 1.0) / 2.0) * (1.0 - ef_t)) + ef_t)
                signal *= ((((sy + 1.0) / 2.0) * (1.0 - ef_t)) + ef_t)
            if r < 1.2:
                r = 1.2
            signal *= sigscalxy
            if signal < 0:
                signal = 0.0
            elif signal > 32:
                signal = 32.0
            if signal == 0:
                continue
            px = ((sx + 1.0) * dw) / 2
            py = ((sy + 1.0) * dh) / 2
            signal /= r
            iy, ymax = int(math.floor(py - r)), int(math.floor(py + r))
            xmin, xmax = int(math.floor(px - r)), int(math.ceil(px + r))
            while iy <= ymax:
                for ix in range(xmin, xmax + 1):
                    if 0 <= ix < dw and 0 <= iy < dh:
                        ddx = ix - px
                        ddy = iy - py
                        fv = signal * ((r - math.sqrt((ddx * ddx) + (ddy * ddy))) / r)
                        if fv <= 0:
                            continue
                        acc[iy * dw + ix] = (acc[iy * dw + ix] + int(fv * 255)) & 0xFFFFFFFF
                iy += 1
    acc = np.array(acc, dtype=np.uint32).reshape(dh, dw)
    return acc, bgra_of(acc, field)
