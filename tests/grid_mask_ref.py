"""numpy restatements for the GridMask tests: the mask (closed form, and loop for loop as the reference builds it), its application,
and the device route's draws (graph-detr4d_amd/csrc/gd4d_grid_mask_rng.h restated with Python integers).  No GPU, no package import."""
import numpy as np

M32 = 0xFFFFFFFF


def mask_closed(h, w, d, l, st_h, st_w, use_h=True, use_w=True, mode=0):
    """The cropped mask (h, w) float32 as include/gd4d.h states it: hh = int(1.5 h), Y = y + (hh - h) // 2, row y is in a band iff
    use_h, k = Y - st_h >= 0, k // d < hh // d and k % d < l (columns: ww, st_w, use_w); 0 in a band row or column, 1 elsewhere;
    mode 1 inverts."""
    def axis(n, st, use):
        nn = int(1.5 * n)
        k = np.arange(n) + (nn - n) // 2 - st
        return use & (k >= 0) & (k // d < nn // d) & (k % d < l)
    band = axis(h, st_h, bool(use_h))[:, None] | axis(w, st_w, bool(use_w))[None, :]
    mask = np.where(band, 0.0, 1.0).astype(np.float32)
    return 1 - mask if mode == 1 else mask


def mask_literal(h, w, d, l, st_h, st_w, use_h=True, use_w=True, mode=0):
    """The same mask the way models/utils/grid_mask.py builds it, loop for loop, for the angle 0 (PIL's rotate(0) returns the array
    unchanged): the big array (:89-90, 93), hh // d row bands (:96-100), ww // d column bands (:101-105), the uint8 round trip
    (:108-110), the centre crop (:111), the inversion (:114-115)."""
    hh, ww = int(1.5 * h), int(1.5 * w)                                     # :89-90
    mask = np.ones((hh, ww), np.float32)                                    # :93
    if use_h:                                                               # :96
        for i in range(hh // d):                                            # :97
            s = d * i + st_h                                                # :98
            t = min(s + l, hh)                                              # :99
            mask[s:t, :] *= 0                                               # :100
    if use_w:                                                               # :101
        for i in range(ww // d):                                            # :102
            s = d * i + st_w                                                # :103
            t = min(s + l, ww)                                              # :104
            mask[:, s:t] *= 0                                               # :105
    mask = np.uint8(mask)                                                   # :108-110 at angle 0
    mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]          # :111
    mask = mask.astype(np.float32)                                          # :113
    if mode == 1:                                                           # :114
        mask = 1 - mask                                                     # :115
    return mask


def apply_ref(x, mask, offset=None):
    """x (..., h, w) float32 through the mask: x * mask, or with an offset map x where mask == 1 and offset where mask == 0
    (:116-121: x * mask + offset * (1 - mask) with a 0 / 1 mask)."""
    x = np.asarray(x, dtype=np.float32)
    if offset is None:
        return np.where(mask == 1, x, np.float32(0))
    return np.where(mask == 1, x, np.asarray(offset, dtype=np.float32))


# ---- the device route's draws: csrc/gd4d_grid_mask_rng.h --------------------------------------------------------------------------
def fmix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def gm_hash(seed, step, i):
    lo, hi = seed & M32, (seed >> 32) & M32
    key = fmix(((step + 0x9E3779B9) & M32) ^ hi)
    return fmix(((((i & M32) ^ lo) * 0x9E3779B1) + key) & M32)


def prob_threshold(prob):
    t = float(prob) * 4294967296.0
    return 0 if t <= 0.0 else (M32 if t >= 4294967295.0 else int(t + 0.5))


def device_draw_ref(seed, step, thresh, h, ratio):
    """(apply, d, l, st_h, st_w) of step `step`."""
    apply = 1 if (thresh == M32 or gm_hash(seed, step, M32) < thresh) else 0
    d = 2 + (((h - 2) * gm_hash(seed, step, M32 - 1)) >> 32)
    l = min(max(int(d * ratio + 0.5), 1), d - 1)
    st_h = (d * gm_hash(seed, step, M32 - 2)) >> 32
    st_w = (d * gm_hash(seed, step, M32 - 3)) >> 32
    return apply, d, l, st_h, st_w


def device_step_ref(state, h, ratio):
    """gd4d_grid_mask_draw on the host: state = [seed_lo, seed_hi, step, thresh] -> (the 8-word block it writes, the state it leaves:
    the step counter one further, mod 2^32)."""
    lo, hi, step, thresh = state
    block = list(device_draw_ref(lo | (hi << 32), step, thresh, h, ratio)) + [lo, hi, step]
    return block, [lo, hi, (step + 1) & M32, thresh]


def device_offset_ref(seed, step, h, w):
    """The (h, w) float32 offset map of step `step`: (hash(seed, step, y w + x) >> 8) 2^-23 - 1, vectorised."""
    lo, hi = seed & M32, (seed >> 32) & M32
    key = np.uint64(fmix(((step + 0x9E3779B9) & M32) ^ hi))
    m = np.uint64(M32)
    x = ((np.arange(h * w, dtype=np.uint64) ^ np.uint64(lo)) * np.uint64(0x9E3779B1) + key) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return ((x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1)).reshape(h, w)


# ---- tests/golden/grid_mask.npz (tools/gen_golden_grid_mask.py) ----------------------------------------------------------------------
_CASES = None


def fixture_cases():
    """The fixture's cases, loaded once: the meta of each plus `x` (float32 input) and `y` (the reference's output; None when the gate
    returned the input)."""
    global _CASES
    if _CASES is None:
        from golden_io import Golden
        g = Golden('grid_mask')
        scale = np.float32(g.meta['scale'])
        _CASES = []
        for i, c in enumerate(g.meta['cases']):
            h, w = c['shape'][-2:]
            x = g.arrays[f'x_{h}x{w}@q'].astype(np.float32) / scale
            y = None
            if f'y{i}' in g.arrays:
                y = g.arrays[f'y{i}']
            elif f'y{i}@q' in g.arrays:
                y = g.arrays[f'y{i}@q'].astype(np.float32) / scale
            _CASES.append(dict(c, x=x, y=y))
    return _CASES
