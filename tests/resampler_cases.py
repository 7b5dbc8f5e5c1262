"""Shared pieces of the plain-resampler tests (tests/test_resampler_host.py, tests/test_gpu_resampler.py): the reference's
rotation case (multi_view_model/tests/test_resampler.py) and small graphs that route through the three resample_layer
paths, each with a numpy-oracle twin."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ------------------------------------------------------------------------------------------------ the reference's case
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _decode_png_rgb8(raw):
    """8-bit RGB, non-interlaced PNG -> uint8 [H, W, 3] (the only kind this needs)."""
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    i, idat, hdr = 8, b'', None
    while i < len(raw):
        n, kind = struct.unpack('>I4s', raw[i:i + 8])
        body = raw[i + 8:i + 8 + n]
        if kind == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat += body
        i += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and ctype == 2 and interlace == 0, hdr
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int32)
    prev = np.zeros(3 * w, np.int32)
    for y in range(h):
        f, line = rows[y, 0], rows[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f in (1, 3, 4):
            # left-dependent filters: one pixel (3 bytes) at a time
            cur = np.zeros(3 * w, np.int32)
            for x in range(0, 3 * w, 3):
                left = cur[x - 3:x] if x else np.zeros(3, np.int32)
                up = prev[x:x + 3]
                ul = prev[x - 3:x] if x else np.zeros(3, np.int32)
                pred = left if f == 1 else ((left + up) >> 1 if f == 3 else _paeth(left, up, ul))
                cur[x:x + 3] = (line[x:x + 3] + pred) & 255
        else:
            raise ValueError("PNG filter %d" % f)
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3).astype(np.uint8)


def rectangle_image():
    """tests/golden/rectangle.png (the input of the reference's resampler test) as uint8 [1500, 2100, 3]."""
    path = os.path.join(GOLDEN, 'rectangle.png')
    try:
        from PIL import Image
        img = np.asarray(Image.open(path).convert('RGB'))
    except ImportError:
        with open(path, 'rb') as f:
            img = _decode_png_rgb8(f.read())
    return np.ascontiguousarray(img)


def rotation_warp(h=1500, w=2100, angle=10.0):
    """test_resampler.py:24-40 in fp32: meshgrid 'ij', [X, Y] @ [[c, -s], [s, c]], x clipped to [0, w], y to [0, h];
    returns [1, h, w, 2] (x, y)."""
    rads = np.radians(angle)
    c, s = np.cos(rads), np.sin(rads)
    rot = np.array([[c, -s], [s, c]], np.float32)
    Y, X = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    pts = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
    wp = (pts @ rot).astype(np.float32)
    wx = np.clip(wp[:, 0].reshape(h, w), 0, w).astype(np.float32)
    wy = np.clip(wp[:, 1].reshape(h, w), 0, h).astype(np.float32)
    return np.stack([wx, wy], axis=2)[None]


# ------------------------------------------------------------------------------------------------ graphs
N, H, W, HS, WS = 2, 12, 10, 9, 14          # warp grid H x W over a Hs x Ws source (non-square, Hs != Ws)
S = 10                                      # warp_pts_src: flow and source are S x S (coords index the transposed grid)


def graph_feeds(rng, case):
    """Inputs of graph_case / oracle_case `case` ('conv_warp', 'conv_src', 'warp_pts_src')."""
    hw = (S, S) if case == 'warp_pts_src' else (H, W)
    f = {'img': rng.uniform(0, 1, (N, S, S, 3) if case == 'warp_pts_src' else (N, HS, WS, 3)).astype(np.float32),
         'tgt': rng.uniform(0, 1, (N,) + hw + (4 if case != 'conv_warp' else 3,)).astype(np.float32)}
    if case == 'conv_warp':
        # feature map whose first two channels are a (column, row) grid over the source: the conv turns it into a warp
        yy, xx = np.meshgrid(np.linspace(-1.5, HS + 0.5, H), np.linspace(-1.5, WS + 0.5, W), indexing='ij')
        feat = rng.normal(0, 1, (N, H, W, 4)).astype(np.float32)
        feat[..., 0] = xx
        feat[..., 1] = yy
        f['feat'] = feat
    if case == 'conv_src':
        f['warp'] = np.stack([rng.uniform(-1.5, WS + 0.5, (N, H, W)), rng.uniform(-1.5, HS + 0.5, (N, H, W))], -1).astype(np.float32)
    return f


def graph_variables(rng, case):
    """Variables that make the conv_warp case sample all over the source: w = identity on the grid channels + noise."""
    if case != 'conv_warp':
        return None
    w = rng.normal(0, 0.05, (3, 3, 4, 2)).astype(np.float32)
    w[1, 1, 0, 0] += 1.0
    w[1, 1, 1, 1] += 1.0
    return {'warpconv/w': w, 'warpconv/b': rng.normal(0, 0.3, (2,)).astype(np.float32)}


def build_graph(tf, g, case):
    """The graph of `case` with this package's tf_utils inside `with Graph(...) as g`; returns the named tensors."""
    img = g.placeholder((N, S, S, 3) if case == 'warp_pts_src' else (N, HS, WS, 3), 'img')
    out = {}
    if case == 'conv_warp':
        feat = g.placeholder((N, H, W, 4), 'feat')
        warp = tf.conv2d_msra(feat, 2, 3, 3, 1, 1, 'warpconv')
        gen = tf.resample_layer(img, warp)
        tgt = g.placeholder((N, H, W, 3), 'tgt')
    elif case == 'conv_src':
        src = tf.tanh(tf.conv2d_msra(img, 4, 3, 3, 1, 1, 'srcconv'))
        warp = g.placeholder((N, H, W, 2), 'warp')
        gen = tf.resampler(src, warp)
        tgt = g.placeholder((N, H, W, 4), 'tgt')
        out['src'] = src
    else:
        src = tf.tanh(tf.conv2d_msra(img, 4, 3, 3, 1, 1, 'srcconv'))
        flow = tf.conv2d_msra(img, 2, 3, 3, 1, 1, 'flowconv')
        warp = tf.warp_pts_layer(flow)
        gen = tf.resample_layer(src, warp)
        tgt = g.placeholder((N, S, S, 4), 'tgt')
        out['src'] = src
        out['flow'] = flow
    out['warp'], out['gen'] = warp, gen
    g.loss_expr = tf.euclidean_loss(gen, tgt)
    g.lr = 1e-4
    return out


def oracle_builder(case):
    """The same graph on the oracle tape (oracle/graph.py)."""
    def build(t, n):
        img, tgt = n['img'], n['tgt']
        out = {}
        if case == 'conv_warp':
            warp = t.conv2d_msra(n['feat'], 2, 3, 3, 1, 1, 'warpconv')
            gen = t.resample_layer(img, warp)
        elif case == 'conv_src':
            src = t.tanh(t.conv2d_msra(img, 4, 3, 3, 1, 1, 'srcconv'))
            warp = n['warp']
            gen = t.resample_layer(src, warp)
            out['src'] = src
        else:
            src = t.tanh(t.conv2d_msra(img, 4, 3, 3, 1, 1, 'srcconv'))
            flow = t.conv2d_msra(img, 2, 3, 3, 1, 1, 'flowconv')
            warp = t.warp_pts_layer(flow)
            gen = t.resample_layer(src, warp)
            out['src'], out['flow'] = src, flow
        out['warp'], out['gen'] = warp, gen
        out['loss'] = t.euclidean_loss(gen, tgt)
        return out
    return build
