"""Seeded tables for the scored box evaluation (K24): ground truth and detections for the matching entry, (class, score, mask)
columns for the accumulation entry.  Everything is a function of its seed."""
import numpy as np

# the matching kernel's tiles (csrc/k24_eval.hip): 16 GT boxes x 32 detections per 16-lane group, 64 x 128 per wave
TILES = ((16, 32), (64, 128))
ACC_TILE = 256          # positions per step of the accumulation's walk


def boxes(rng, n):
    """rounded boxes, 30 % with swapped corners (as the comparison's tests make them)"""
    c = rng.uniform(0, 200, (n, 2))
    box4 = np.round(np.concatenate([c, c + rng.uniform(1, 60, (n, 2))], axis=1), 1)
    swap = rng.random(n) < 0.3
    box4[swap] = box4[swap][:, [2, 3, 0, 1]]
    return box4


def match_table(sizes, seed, n_classes=3, special=True):
    """sizes = [(n_gt, n_dt)] per row -> (gt_box4, gt_off, gt_cls, dt_box4, dt_off, dt_cls, dt_score, n_classes).  Detections are
    copies of a GT box of their row shrunk to an IoU of 1, 0.93, 0.8, 0.65 or 0.52 (so that the free sets differ between the
    thresholds), 5 % of them under another class, plus unrelated boxes; scores have two decimals, so ties are common.  With
    `special`, NaN / inf corners and NaN, +-inf and -0.0 scores are planted."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    g_off, d_off = np.zeros(len(sizes) + 1, np.int32), np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(sizes[:, 0], out=g_off[1:])
    np.cumsum(sizes[:, 1], out=d_off[1:])
    ng, nd = int(g_off[-1]), int(d_off[-1])
    g, d = boxes(rng, ng), boxes(rng, nd)
    g_cls = rng.integers(0, n_classes, ng).astype(np.int32)
    d_cls = rng.integers(0, n_classes, nd).astype(np.int32)
    shrink = np.asarray([1.0, 0.93, 0.8, 0.65, 0.52])
    for r in range(len(sizes)):
        if g_off[r + 1] == g_off[r]:
            continue
        for j in range(d_off[r], d_off[r + 1]):
            if rng.random() < 0.8:
                i = rng.integers(g_off[r], g_off[r + 1])
                d[j], d_cls[j] = g[i], g_cls[i]
                d[j, 3] = d[j, 1] + (d[j, 3] - d[j, 1]) * shrink[rng.integers(0, len(shrink))]
                if rng.random() < 0.05 and n_classes > 1:
                    d_cls[j] = (d_cls[j] + 1) % n_classes
    score = np.round(rng.random(nd), 2)
    if special:
        vals = [np.nan, np.inf, -np.inf, -0.0]
        for t in (g, d):
            if len(t) >= 8:
                for k, q in enumerate(rng.choice(len(t), max(4, len(t) // 50), replace=False)):
                    t[q, k % 4] = vals[k % 4]
        if nd >= 8:
            for k, q in enumerate(rng.choice(nd, max(4, nd // 40), replace=False)):
                score[q] = vals[k % 4]
    return g, g_off, g_cls, d, d_off, d_cls, score, n_classes


def dense_table(seed, n_rows=2000, max_boxes=12, n_classes=3):
    """jittered copies: every GT box has a detection shrunk to one of the IoU steps, half of the detections come a second time
    with a lower score, 5 % are relabelled"""
    rng = np.random.default_rng(seed)
    n_g = rng.integers(0, max_boxes + 1, n_rows)
    g_off = np.zeros(n_rows + 1, np.int32)
    np.cumsum(n_g, out=g_off[1:])
    g = boxes(rng, int(g_off[-1]))
    g_cls = rng.integers(0, n_classes, len(g)).astype(np.int32)
    shrink = np.asarray([1.0, 0.93, 0.8, 0.65, 0.52])
    d, d_cls, score, counts = [], [], [], []
    for r in range(n_rows):
        k = 0
        for i in range(g_off[r], g_off[r + 1]):
            b = g[i].copy()
            b[3] = b[1] + (b[3] - b[1]) * shrink[rng.integers(0, len(shrink))]
            c = int(g_cls[i]) if rng.random() >= 0.05 else (int(g_cls[i]) + 1) % n_classes
            s = round(float(rng.random()), 2)
            d.append(b), d_cls.append(c), score.append(s)
            k += 1
            if rng.random() < 0.5:
                b2 = b.copy()
                b2[2] = b2[0] + (b2[2] - b2[0]) * shrink[rng.integers(0, len(shrink))]
                d.append(b2), d_cls.append(c), score.append(round(s * float(rng.random()), 2))
                k += 1
        counts.append(k)
    d_off = np.zeros(n_rows + 1, np.int32)
    np.cumsum(counts, out=d_off[1:])
    return (g, g_off, g_cls, np.asarray(d, np.float64).reshape(-1, 4), d_off, np.asarray(d_cls, np.int32),
            np.asarray(score, np.float64), n_classes)


def acc_table(segments, seed, T, decimals=2):
    """segments = detections per class -> (cls, score, tp, n_classes, T, npig): shuffled over the table, masks with about 60 % of
    the bits set at the first threshold and fewer at the later ones, scores of `decimals` decimals (ties), npig between the TPs
    of the class and twice that; a class without detections keeps a GT box, the last class with detections has none"""
    rng = np.random.default_rng(seed)
    C = len(segments)
    cls = np.repeat(np.arange(C, dtype=np.int32), segments)
    rng.shuffle(cls)
    n = len(cls)
    score = np.round(rng.random(n), decimals)
    if n:
        score[rng.integers(0, n, max(1, n // 100))] = -0.0
    tp = np.zeros(n, np.uint32)
    u = rng.random(n)
    for t in range(T):
        tp |= (u < 0.6 * (1 - t / (T + 1))).astype(np.uint32) << np.uint32(t)
    npig = np.zeros(C, np.int64)
    for c in range(C):
        most = int((tp[cls == c] & 1).sum())
        npig[c] = most + int(rng.integers(0, most + 2)) if segments[c] else 3
    if C >= 2 and segments[-1]:
        npig[-1] = 0
    return cls, score, tp, C, T, npig
