"""The numpy statement of the connected components (include/microaligner_components.h), written from the definitions: the
neighbour relation as a list of pixel pairs, a union-find over it whose roots are the smallest linear index of every class,
numbering by that index.  It does not call scipy; tests/test_components_ref.py holds it against scipy.ndimage.  Also the
patterns the tests label."""
import numpy as np

T = 64                      # the tile of csrc/components.hip (MA_CC_TILE): the patterns put their seams there
DTYPES = (np.uint8, np.uint16, np.int32)


# ---- the statement --------------------------------------------------------------------------------------------------------
def _pairs(key, connectivity):
    """the joined pairs (a, b) of linear indices: neighbours under `connectivity` whose keys are equal and not 0"""
    H, W = key.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    offsets = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 2 else [])
    A, B = [], []
    for dy, dx in offsets:
        ya, yb = slice(0, H - dy), slice(dy, H)
        xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        m = (key[ya, xa] != 0) & (key[ya, xa] == key[yb, xb])
        A.append(idx[ya, xa][m])
        B.append(idx[yb, xb][m])
    return np.concatenate(A), np.concatenate(B)


def _roots(key, connectivity):
    """root[p]: the smallest linear index of the class of p under the transitive closure of the pairs"""
    assert connectivity in (1, 2)
    A, B = _pairs(key, connectivity)
    parent = np.arange(key.size, dtype=np.int64)
    while True:
        while True:                                  # every pixel to its root
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        ra, rb = parent[A], parent[B]
        d = ra != rb
        if not d.any():
            return parent
        A, B, ra, rb = A[d], B[d], ra[d], rb[d]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))      # the larger root under the smaller


def _key(img, by_value):
    img = np.asarray(img)
    assert img.ndim == 2
    return img.astype(np.int64) if by_value else (img != 0).astype(np.int64)


def label_ref(img, connectivity=1, by_value=False):
    """(labels int32, n): component k = 1 .. n is the k-th in ascending order of the components' smallest linear index"""
    key = _key(img, by_value)
    root = _roots(key, connectivity)
    fg = key.ravel() != 0
    first = np.flatnonzero(fg & (root == np.arange(key.size)))             # ascending
    rank = np.zeros(key.size, np.int64)
    rank[first] = np.arange(1, first.size + 1)
    return np.where(fg, rank[root], 0).astype(np.int32).reshape(key.shape), int(first.size)


def stats_ref(labels, n):
    """(areas int64 (n + 1,), bboxes int32 (n + 1, 4)): y0, x0, y1, x1 with the ends exclusive; row 0 and absent labels zeros"""
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels <= n)
    areas = np.bincount(labels[ok].ravel(), minlength=n + 1).astype(np.int64)
    ys, xs = np.nonzero(ok & (labels > 0))
    lab = labels[ys, xs]
    big = np.iinfo(np.int64).max
    box = np.stack([np.full(n + 1, big), np.full(n + 1, big), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)], axis=1)
    np.minimum.at(box[:, 0], lab, ys)
    np.minimum.at(box[:, 1], lab, xs)
    np.maximum.at(box[:, 2], lab, ys + 1)
    np.maximum.at(box[:, 3], lab, xs + 1)
    box[areas == 0] = 0
    box[0] = 0
    return areas, box.astype(np.int32)


def remove_small_ref(img, min_size, connectivity=1, by_value=False):
    img = np.asarray(img)
    labels, n = label_ref(img, connectivity, by_value)
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    out = img.copy()
    out[(labels > 0) & (areas[labels] < min_size)] = 0
    return out


def fill_holes_ref(img, max_size=None, connectivity=1, value=1):
    img = np.asarray(img)
    labels, n = label_ref(img == 0, connectivity)
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    hole = np.ones(n + 1, bool)
    hole[0] = False
    hole[labels[0]] = hole[labels[-1]] = hole[labels[:, 0]] = hole[labels[:, -1]] = False
    if max_size is not None:
        hole &= areas <= max_size
    out = img.copy()
    out[hole[labels]] = value
    return out


def as_dtype(mask, dtype, top=False):
    """a 0/1 pattern in `dtype`: foreground 1, or the dtype's largest value with top"""
    v = np.iinfo(dtype).max if top else 1
    return (np.asarray(mask) != 0).astype(dtype) * dtype(v)


# ---- patterns: all uint8 0/1 -------------------------------------------------------------------------------------------------
def zeros(H, W):
    return np.zeros((H, W), np.uint8)


def ones(H, W):
    return np.ones((H, W), np.uint8)


def random_mask(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def serpentine(H, W):
    """a path one pixel wide through every row: the even rows whole, joined at alternating ends by the odd rows"""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    m[1::4, W - 1] = 1
    m[3::4, 0] = 1
    return m


def spiral(H, W):
    """a path one pixel wide from the corner inwards, one pixel of background between its turns"""
    m = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx
        if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return m


def rings(H, W):
    """concentric square rings one pixel apart: holes inside objects inside holes"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.minimum(np.minimum(yy, xx), np.minimum(H - 1 - yy, W - 1 - xx)) % 2 == 0).astype(np.uint8)


def main_diagonal(H, W):
    """(i, i): consecutive pixels meet at the tile corner between (T - 1, T - 1) and (T, T)"""
    m = np.zeros((H, W), np.uint8)
    i = np.arange(min(H, W))
    m[i, i] = 1
    return m


def anti_diagonal(H, W):
    """(i, 2 T - 1 - i): it crosses the tile corner between (T - 1, T) and (T, T - 1)"""
    m = np.zeros((H, W), np.uint8)
    i = np.arange(H)
    x = 2 * T - 1 - i
    ok = (x >= 0) & (x < W)
    m[i[ok], x[ok]] = 1
    return m


def u_and_j(H, W):
    """a U whose smallest pixel is the top of its right arm, and a J inside it whose smallest pixel is the top of its stem:
    each in another tile than most of its pixels.  Needs H >= 40, W >= 60."""
    m = np.zeros((H, W), np.uint8)
    l, r, b = 3, W - 4, H - 3
    m[9:b + 1, l] = 1
    m[b, l:r + 1] = 1
    m[2:b + 1, r] = 1
    s, jb, e = W - 12, H - 8, 10
    m[5:jb + 1, s] = 1
    m[jb, e:s + 1] = 1
    m[jb - 15:jb + 1, e] = 1
    return m


def border_holes(H, W):
    """foreground with holes (zeros): one that touches each border line at exactly one pixel, one that reaches each corner
    pixel only across a diagonal (enclosed under 4 neighbours, open under 8), and two that are enclosed.  Needs H, W >= 32."""
    m = np.ones((H, W), np.uint8)
    cy, cx = H // 2, W // 2
    m[1:4, cx - 1:cx + 2] = 0
    m[0, cx] = 0                               # row 0
    m[H - 4:H - 1, cx - 1:cx + 2] = 0
    m[H - 1, cx + 1] = 0                       # row H - 1
    m[cy - 1:cy + 2, 1:4] = 0
    m[cy, 0] = 0                               # column 0
    m[cy - 1:cy + 2, W - 4:W - 1] = 0
    m[cy - 1, W - 1] = 0                       # column W - 1
    for y, x, by, bx in ((0, 0, 1, 1), (0, W - 1, 1, W - 3), (H - 1, 0, H - 3, 1), (H - 1, W - 1, H - 3, W - 3)):
        m[y, x] = 0
        m[by:by + 2, bx:bx + 2] = 0
    m[cy - 6:cy - 3, cx - 6:cx + 6] = 0        # enclosed
    m[cy + 5, cx] = 0                          # enclosed, one pixel
    return m


def sized_blobs(H, W, size, value=1, back=0):
    """two blobs of `value` on `back`, of exactly `size` and `size + 1` pixels, neither a rectangle, apart from each other
    and from the border.  Needs H >= 8, W >= 2 * size + 8."""
    m = np.full((H, W), back, np.uint8)
    m[2, 2:2 + size - 1] = value
    m[3, 2] = value                            # size
    m[5, 3:3 + size] = value
    m[6, 3 + size - 1] = value                 # size + 1
    return m
