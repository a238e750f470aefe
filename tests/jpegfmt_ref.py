"""numpy restatement of the JPEG decoder's layout family (attwarp_amd/csrc/jpegfmt_blocks.hpp, the jpegfmt_* kernels of
jpegdec.hip) on top of jpegdec_ref: the marker walk with libjpeg's colour rule, the general-MCU entropy
walk, the IDCT over up to four planes, the up-sampler jdsample.c picks per component, the four colour rules and Pillow's
conversions.  Pinned to Pillow by tests/test_jpegfmt_ref_cpu.py; the kernels and the host program are compared with it."""
from __future__ import annotations

import io
import struct

import numpy as np
from PIL import Image

import jpegdec_ref as D

MAX_SLOTS = 10


def parse(data):
    """The marker walk of a well-formed sequential file of ANY layout -> dict(W, H, ncomp, samp [(h, v)], color, ri, qt, dc,
    ac, stream).  color: "grey", "ycc", "rgb", "cmyk", "ycck" by libjpeg's rule.  ValueError for what libjpeg refuses in the
    factors; the refusals of the headers are the package's (tests/test_jpegfmt_host_cpu.py)."""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    pos, qts, dcs, acs, ri, jfif, adobe, frame = 2, {}, {}, {}, 0, False, None, None
    while True:
        assert d[pos] == 0xFF
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        L = struct.unpack(">H", d[pos + 1:pos + 3])[0]
        seg = d[pos + 3:pos + 1 + L]
        pos += 1 + L
        if m in (0xC0, 0xC1):
            prec, H, W, nf = struct.unpack(">BHHB", seg[:6])
            assert prec == 8
            frame = (W, H, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                (acs if seg[q] >> 4 else dcs)[seg[q] & 15] = (counts, list(seg[q + 17:q + 17 + sum(counts)]))
                q += 17 + sum(counts)
        elif m == 0xDB:
            for q in range(0, len(seg), 65):
                t = [0] * 64
                for k in range(64):
                    t[D.ZIGZAG[k]] = seg[q + 1 + k]
                qts[seg[q] & 15] = t
        elif m == 0xDD:
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            break
    W, H, comps = frame
    nf = len(comps)
    assert seg[0] == nf and [seg[1 + 2 * i] for i in range(nf)] == [c[0] for c in comps]
    if nf not in (1, 3, 4):
        raise ValueError("jpeg: components")
    samp = [(c[1], c[2]) for c in comps] if nf > 1 else [(1, 1)]            # (one component: not interleaved, factors ignored)
    if any(not 1 <= f <= 4 for hv in samp for f in hv) or sum(h * v for h, v in samp) > MAX_SLOTS:
        raise ValueError("jpeg: sampling factors")
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    if any(hmax % h or vmax % v for h, v in samp):
        raise ValueError("jpeg: fractional up-sampling")
    if nf == 1:
        color = "grey"
    elif nf == 3:                                               # default_decompress_parms of jdapimin.c
        rgb = not jfif and (adobe == 0 if adobe is not None else bytes(c[0] for c in comps) == b"RGB")
        color = "rgb" if rgb else "ycc"
    else:
        color = "cmyk" if adobe in (None, 0) else "ycck"
    tabs = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(nf)]
    return dict(W=W, H=H, ncomp=nf, samp=samp, color=color, ri=ri, qt=[qts[c[3]] for c in comps], dc=[dcs[t[0]] for t in tabs],
                ac=[acs[t[1]] for t in tabs], stream=d[pos:])


def geometry(p):
    samp = p["samp"]
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-p["W"] // (8 * hmax)), -(-p["H"] // (8 * vmax))
    nmcu = mcux * mcuy
    bw, bh = [mcux * h for h, _ in samp], [mcuy * v for _, v in samp]
    slots = [(c, x, y) for c, (h, v) in enumerate(samp) for y in range(v) for x in range(h)]      # the MCU's blocks in file order
    true = [(-(-p["W"] * h // hmax), -(-p["H"] * v // vmax)) for h, v in samp]                     # (dw, dh) per component
    return dict(hmax=hmax, vmax=vmax, mcux=mcux, mcuy=mcuy, nmcu=nmcu, bw=bw, bh=bh, slots=slots, true=true,
                nunits=-(-nmcu // p["ri"]) if p["ri"] else 1, nblocks=sum(a * b for a, b in zip(bw, bh)))


def entropy(p):
    """The general-MCU walk -> (status, [coefficient planes int16 [bh, bw, 64]] per component, info), with the statuses and
    their precedence of jpegdec_ref.entropy."""
    g = geometry(p)
    s = p["stream"]
    st, units, eoi = D.scan(s, g["nunits"])
    planes = [np.zeros((g["bh"][c], g["bw"][c], 64), np.int16) for c in range(p["ncomp"])]
    info = dict(nunits=g["nunits"], eoi=eoi, units=units)
    if st:
        return st, planes, info
    dct, act = [D.code_table(*t) for t in p["dc"]], [D.code_table(*t) for t in p["ac"]]
    ri = p["ri"] or g["nmcu"]
    first = D.OK
    for k, (a, b) in enumerate(units):
        bits = D._Bits(s[a:b])
        pred = [0] * p["ncomp"]
        ust = D.OK
        for m in range(k * ri, min((k + 1) * ri, g["nmcu"])):
            mx, my = m % g["mcux"], m // g["mcux"]
            for c, x, y in g["slots"]:
                h, v = p["samp"][c]
                ust, pred[c] = D.decode_block(bits, dct[c], act[c], pred[c], planes[c][my * v + y, mx * h + x])
                if ust:
                    break
            if ust:
                break
        if ust and not first:
            first = ust                                       # the lowest failing unit's status
    if first:
        return first, planes, info
    return (D.OK if eoi else D.E_NO_EOI), planes, info


def idct_planes(p, planes):
    """Coefficient planes of up to four components -> uint8 planes padded to whole blocks (the arithmetic is jpegdec_ref's)."""
    return D.idct_planes(p, planes)


def upsampler(rx, ry, dw):
    """The routine jinit_upsampler (jdsample.c, fancy up-sampling on) picks for a component rx x ry coarser than the frame and
    dw samples wide."""
    if (rx, ry) == (1, 1):
        return "copy"
    if (rx, ry) in ((2, 1), (2, 2)) and dw > 2:
        return "h2v1" if ry == 1 else "h2v2"
    return "h1v2" if (rx, ry) == (1, 2) else "box"


def upsample(pl, rx, ry, W, H):
    """A component plane cropped to its true size -> int32 [H, W]."""
    p = pl.astype(np.int32)
    dh, dw = p.shape
    how = upsampler(rx, ry, dw)
    if how in ("copy", "h2v1", "h2v2"):
        return D.upsample(pl, rx, ry, W, H)
    if how == "h1v2":                                         # h1v2_fancy_upsample: 3/4 nearer row + 1/4 further, edges repeated
        up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        o = np.empty((2 * dh, dw), np.int32)
        o[0::2] = (3 * p + up + 1) >> 2
        o[1::2] = (3 * p + dn + 2) >> 2
        return o[:H, :W]
    return np.repeat(np.repeat(p, ry, 0), rx, 1)[:H, :W]


def _muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def cmyk_to_rgb(cmyk):
    """Pillow's cmyk2rgb over uint8 [..., 4] -> uint8 [..., 3]."""
    c = cmyk.astype(np.int64)
    nk = 255 - c[..., 3]
    return np.stack([np.clip(nk - _muldiv255(c[..., k], nk), 0, 255) for k in range(3)], -1).astype(np.uint8)


def pixels(p, comp, mode="RGB", order="rgb"):
    """uint8 component planes (padded) -> what Image.open(f).convert(mode) gives; "keep": the file's own channels."""
    g = geometry(p)
    W, H = p["W"], p["H"]
    s = [upsample(comp[c][:dh, :dw], g["hmax"] // p["samp"][c][0], g["vmax"] // p["samp"][c][1], W, H)
         for c, (dw, dh) in enumerate(g["true"])]
    color = p["color"]
    if color == "grey":
        y = s[0].astype(np.uint8)[:, :, None]
        return np.repeat(y, 3, 2) if mode == "RGB" else y
    if color in ("ycc", "ycck"):
        cb, cr = s[1] - 128, s[2] - 128
        rgb = np.stack([s[0] + ((91881 * cr + 32768) >> 16), s[0] + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                        s[0] + ((116130 * cb + 32768) >> 16)], 2)
        rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    else:
        rgb = np.stack(s[:3], 2).astype(np.uint8)
    if p["ncomp"] == 4:
        # Pillow reads libjpeg's CMYK rows as "CMYK;I" (all four inverted); libjpeg gives a YCCK file as 255 - RGB and K as stored
        cmy = rgb if color == "ycck" else 255 - rgb
        cmyk = np.concatenate([cmy, (255 - s[3]).astype(np.uint8)[:, :, None]], 2)
        if mode == "keep":
            return cmyk
        rgb = cmyk_to_rgb(cmyk)
    if mode == "L":
        return D.luma(rgb)[:, :, None]
    return rgb[:, :, ::-1].copy() if order == "bgr" else rgb


def pillow(f, mode="RGB"):
    """Pillow's pixels [H, W, C]; "keep": in the mode Pillow opens the file with (L, RGB or CMYK)."""
    im = Image.open(io.BytesIO(f))
    a = np.asarray(im if mode == "keep" else im.convert(mode))
    return a[:, :, None] if a.ndim == 2 else a


_CACHE = {}


def decode(f, mode="RGB", order="rgb"):
    """A file -> (status, pixels [H, W, C] or None, info).  info: nunits, crc (of the coefficients; 0 unless OK), eoi."""
    key = bytes(f)
    if key not in _CACHE:
        p = parse(key)
        st, planes, info = entropy(p)
        info = dict(info, crc=D.coef_crc(planes) if st == D.OK else 0)
        _CACHE[key] = (p, st, idct_planes(p, planes) if st == D.OK else None, info)
    p, st, comp, info = _CACHE[key]
    if st:
        return st, None, info
    return st, pixels(p, comp, mode, order), info
