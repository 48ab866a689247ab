"""Write tests/golden/cv2_levels_4.5.5.npz: OpenCV's own pyramid Farneback and the two primitives it is built from.

    python tests/golden/make_cv2_levels_golden.py        # numpy + opencv-contrib-python==4.5.5.64, nothing else

Holds, for seeded small pairs (even and odd sizes):
  * cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, levels, win, 3, 1, 1.7, OPTFLOW_FARNEBACK_GAUSSIAN) for
    levels 1..4 and win 15 / 51;
  * cv2.resize(float32, (w_k, h_k), INTER_LINEAR) of the first image at the level sizes of the pyramid (odd ones included)
    and of a 2-channel float32 field upwards by the level ratio, as the flow initialisation does;
  * cv2.GaussianBlur(float32, (ksize_k, ksize_k), sigma_k) at the level sigmas.
tests/test_cv2_levels_golden.py compares the CPU restatement (and, under -m gpu, the HIP path) with it."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cv2_levels_4.5.5.npz")
SHAPES = [(160, 192), (161, 203), (259, 131)]
LEVELS = [1, 2, 3, 4]
WINS = [15, 51]
ITERS = 3


def make_pair(H, W, seed):
    """smooth seeded texture and a copy shifted by (6, -4) px with a little noise, uint8"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H + 16, 0:W + 16].astype(np.float64)
    img = sum(np.sin(x * rng.uniform(0.05, 0.3) + rng.uniform(0, 6)) * np.cos(y * rng.uniform(0.05, 0.3) + rng.uniform(0, 6))
              for _ in range(6))
    img = (img - img.min()) / (img.max() - img.min()) * 200 + 20
    a = img[8:8 + H, 8:8 + W]
    b = img[4:4 + H, 14:14 + W] + rng.normal(0, 1.0, (H, W))
    return np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8)


def level_table(H, W, levels):
    """(w_k, h_k, ksize_k, sigma_k) as FarnebackOpticalFlow::calc forms them"""
    k, scale = 0, 1.0
    while k < levels:
        scale *= 0.5
        if W * scale < 32 or H * scale < 32:
            break
        k += 1
    out = []
    for i in range(k + 1):
        s = 0.5 ** i
        sigma = (1 / s - 1) * 0.5
        out.append((int(round(W * s)), int(round(H * s)), max(int(round(sigma * 5)) | 1, 3), sigma))
    return out


def main():
    import cv2
    assert cv2.__version__.startswith("4.5.5"), cv2.__version__
    d = {"cv2_version": np.array(cv2.__version__)}
    for si, (H, W) in enumerate(SHAPES):
        prev, nxt = make_pair(H, W, 100 + si)
        d[f"s{si}_prev"], d[f"s{si}_next"] = prev, nxt
        for lv in LEVELS:
            for win in WINS:
                d[f"s{si}_flow_l{lv}_w{win}"] = cv2.calcOpticalFlowFarneback(prev, nxt, None, 0.5, lv, win, ITERS, 1, 1.7,
                                                                             cv2.OPTFLOW_FARNEBACK_GAUSSIAN)
        f = prev.astype(np.float32)
        rng = np.random.default_rng(200 + si)
        for k, (w, h, ks, sigma) in enumerate(level_table(H, W, max(LEVELS))):
            if k == 0:
                continue
            d[f"s{si}_blur_k{k}"] = cv2.GaussianBlur(f, (ks, ks), sigma, sigmaY=sigma)
            d[f"s{si}_resize_k{k}"] = cv2.resize(f, (w, h), interpolation=cv2.INTER_LINEAR)
            d[f"s{si}_field_k{k}"] = field = rng.normal(0, 3, (h, w, 2)).astype(np.float32)
            up = level_table(H, W, k - 1)[k - 1] if k > 1 else (W, H)
            d[f"s{si}_fieldup_k{k}"] = cv2.resize(field, (up[0], up[1]), interpolation=cv2.INTER_LINEAR)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
