"""numpy restatement of the court overlay rule (test helper, not a conftest): what sfh_amd.visualize / csrc/overlay.hip must
give byte for byte.  Written from the rule as the project states it (include/sfh_amd.h, sfh_amd/visualize.py), not from the
reference's text: the reference's own ``overlay`` needs OpenCV, which is absent here, so - as for the Kornia leg of the
warp - this is a restatement.

* warp leg: ``oracle.warp_ref``'s nearest warp of the id template, times mask_classes, truncated to int32;
* segmentation leg: int / uint8 ids or logits (first maximum wins) resized with OpenCV's INTER_NEAREST index rule
  ``min(floor(dx * ifx), ws - 1)`` with ``ifx = 1 / (wd / ws)`` in double (``oracle.post_ref.resize_nearest``: the rule of
  sfh_mask_format_fwd; it equals ``dx * (ws / wd)`` wherever ws / wd is exact in double, which covers every case tested);
* palette (ids outside 0..7 count as 0), the integer blend, the disc rule and the glyph table.
"""
import numpy as np
import torch

from oracle import post_ref, warp_ref

PALETTES = {
    4: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255)},
    7: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 4: (255, 255, 255), 5: (255, 0, 255), 6: (0, 255, 255)},
    8: {1: (0, 255, 0), 2: (255, 0, 0), 3: (0, 0, 255), 4: (255, 255, 255), 5: (255, 0, 255), 6: (0, 255, 255),
        7: (255, 255, 0)},
}

CHARSET = "0123456789.-+e naif"
# 5x7 font, rows top to bottom, '#' = lit
_FONT = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    ".": (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),
    "-": (".....", ".....", ".....", "#####", ".....", ".....", "....."),
    "+": (".....", "..#..", "..#..", "#####", "..#..", "..#..", "....."),
    "e": (".....", ".....", ".###.", "#...#", "#####", "#....", ".###."),
    " ": (".....", ".....", ".....", ".....", ".....", ".....", "....."),
    "n": (".....", ".....", "#.##.", "##..#", "#...#", "#...#", "#...#"),
    "a": (".....", ".....", ".###.", "....#", ".####", "#...#", ".####"),
    "i": ("..#..", ".....", ".##..", "..#..", "..#..", "..#..", ".###."),
    "f": ("..##.", ".#..#", ".#...", "###..", ".#...", ".#...", ".#..."),
}


def glyph_rows(ch):
    """the 7 row bytes of a character, bit 4 = leftmost column"""
    return tuple(sum(1 << (4 - c) for c in range(5) if row[c] == "#") for row in _FONT[ch])


def palette(n_classes):
    pal = np.zeros((8, 3), dtype=np.uint8)
    for k, c in PALETTES[n_classes].items():
        pal[k] = c
    return pal


def blend(frame, colour):
    """integer blend of uint8 arrays (...,3): black colour keeps the frame, else (colour + frame) >> 1 per channel"""
    f = frame.astype(np.uint16)
    c = colour.astype(np.uint16)
    keep = (colour == 0).all(axis=-1, keepdims=True)
    return np.where(keep, frame, ((c + f) >> 1).astype(np.uint8))


def warp_ids(theta, template, h, w, mask_classes, shared=False):
    """theta (B,3,3)|(B,1,3,3), template (N,1,ht,wt) float32 torch tensors -> int32 ids (B,h,w)"""
    B = theta.shape[0]
    t = template[0:1].expand(B, -1, -1, -1) if shared or template.shape[0] == 1 else template[:B]
    m = warp_ref.homography_warp(theta.reshape(B, 1, 3, 3).float(), t.float(), h, w, "nearest")
    return (m * np.float32(mask_classes)).to(torch.int32).numpy()


def segm_ids(segm, h, w):
    """ids (B,hs,ws) int or logits (B,nc,hs,ws) float32 (numpy) -> int64 ids (B,h,w)"""
    segm = np.asarray(segm)
    if segm.ndim == 4:
        segm = np.argmax(segm, axis=1)         # the first maximum wins
    return np.stack([post_ref.resize_nearest(m, (w, h)) for m in segm]).astype(np.int64)


def colours(ids, pal):
    ids = np.asarray(ids).astype(np.int64)
    ids = np.where((ids >= 0) & (ids < 8), ids, 0)
    return pal[ids]


def render(frames, theta=None, template=None, mask_classes=4, score=None, segm=None, score_threshold=0.1,
           overlay_threshold=None, source="auto", shared=False):
    """frames uint8 (B,H,W,3) numpy; theta / template torch CPU tensors; score (B,) float32 numpy or None; segm numpy or None"""
    frames = np.asarray(frames)
    B, H, W = frames.shape[:3]
    pal = palette(mask_classes)
    out = frames.copy()
    wids = None
    for b in range(B):
        sc = np.float32(score[b]) if score is not None else None
        thr = np.float32(score_threshold)
        use_warp = source == "warp" or (source == "auto" and bool(sc < thr))
        if use_warp:
            if wids is None:
                wids = warp_ids(theta, template, H, W, mask_classes, shared)
            ids = wids[b]
        elif segm is not None:
            ids = segm_ids(segm[b:b + 1], H, W)[0]
        else:
            continue                            # no mask: the frame is copied
        if overlay_threshold is not None and not bool(sc < np.float32(overlay_threshold)):
            continue
        out[b] = blend(frames[b], colours(ids, pal))
    return out


def marker_centre(p, H, W):
    """(cx, cy) of a normalised point, or None where it draws nothing"""
    x, y = float(p[0]) * W, float(p[1]) * H        # exact in double
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    cx, cy = np.rint(x), np.rint(y)                # ties to even
    if not (abs(cx) < 1e9 and abs(cy) < 1e9):
        return None
    return int(cx), int(cy)


def annotate(img, poi=None, radius=0, marker_color=(255, 255, 255), labels=None, label_pos=(15, 15), label_scale=2,
             score=None, score_threshold=0.1, source="auto"):
    """draws in place on img uint8 (B,H,W,3): markers in point order (a later one over an earlier one), then the label"""
    B, H, W = img.shape[:3]
    for b in range(B):
        if poi is not None and radius > 0:
            for p in np.asarray(poi[b]):
                c = marker_centre(p, H, W)
                if c is None:
                    continue
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        x, y = c[0] + dx, c[1] + dy
                        if dx * dx + dy * dy <= radius * radius and 0 <= x < W and 0 <= y < H:
                            img[b, y, x] = marker_color
        if labels is not None:
            if score is not None:
                low = bool(np.float32(score[b]) < np.float32(score_threshold))
            else:
                low = source == "warp"
            colour = (0, 255, 0) if low else (0, 0, 255)
            for i, ch in enumerate(labels[b]):
                rows = glyph_rows(ch)
                for gy in range(7):
                    for col in range(5):
                        if not (rows[gy] >> (4 - col)) & 1:
                            continue
                        x0 = label_pos[0] + (i * 6 + col) * label_scale
                        y0 = label_pos[1] + gy * label_scale
                        for y in range(max(y0, 0), min(y0 + label_scale, H)):
                            for x in range(max(x0, 0), min(x0 + label_scale, W)):
                                img[b, y, x] = colour
    return img


class StubRenderer:
    """OverlayRenderer's call signature on host arrays (tests of visualize() without a GPU)"""

    def __init__(self, court_img, mask_classes=4, score_threshold=0.1, overlay_threshold=None, source="auto",
                 label_pos=(15, 15), label_scale=2):
        self.kw = dict(template=court_img, mask_classes=mask_classes, score_threshold=score_threshold,
                       overlay_threshold=overlay_threshold, source=source, shared=court_img.shape[0] == 1)
        self.label_pos, self.label_scale = label_pos, label_scale
        self.calls = []

    def __call__(self, frames_u8, theta, score=None, segm=None, poi=None, labels=None, out=None):
        sc = score.cpu().numpy() if score is not None else None
        img = render(frames_u8.cpu().numpy(), theta.cpu(), score=sc, segm=segm.cpu().numpy() if segm is not None else None,
                     **self.kw)
        annotate(img, labels=labels, label_pos=self.label_pos, label_scale=self.label_scale, score=sc,
                 score_threshold=self.kw["score_threshold"], source=self.kw["source"])
        self.calls.append(int(frames_u8.shape[0]))
        return img
