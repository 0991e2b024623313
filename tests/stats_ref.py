"""Independent numpy restatement of the search statistics.  Never calls the library: the tests compare the
kernel, the host library and the command line against this file."""
import numpy as np

LBINS, SBINS = 64, 256
OK, NO_FIT = 0, 1
EULER_GAMMA = 0.5772156649015329


def length_bin(length):
    """Half octaves: e = floor(log2 L), bin = 2 e + (the bit below the leading one); L <= 1 -> 0."""
    length = int(length)
    if length <= 1:
        return 0
    e = length.bit_length() - 1
    return 2 * e + ((length >> (e - 1)) & 1)


def length_bins(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    out = np.zeros(len(lengths), dtype=np.int64)
    big = lengths > 1
    l = lengths[big]
    e = np.floor(np.log2(l.astype(np.float64))).astype(np.int64)
    # float log2 may be off by one next to a power of two: settle it with integers
    e = np.where((np.int64(1) << e) > l, e - 1, e)
    e = np.where((np.int64(1) << (e + 1)) <= l, e + 1, e)
    out[big] = 2 * e + ((l >> (e - 1)) & 1)
    return out


def histogram(scores, lengths):
    """-> (hist uint32 [64][256], sumlen uint64 [64], skipped) of integer-valued scores and true lengths."""
    scores = np.asarray(scores)
    lengths = np.asarray(lengths, dtype=np.int64)
    binned = scores >= 0
    skipped = int(len(scores) - binned.sum())
    s = np.minimum(scores[binned].astype(np.int64), SBINS - 1)
    b = length_bins(lengths[binned])
    hist = np.zeros((LBINS, SBINS), dtype=np.int64)
    np.add.at(hist, (b, s), 1)
    sumlen = np.zeros(LBINS, dtype=np.int64)
    np.add.at(sumlen, b, np.maximum(lengths[binned], 0))
    return hist.astype(np.uint32), sumlen.astype(np.uint64), skipped


def fit(hist, sumlen):
    """-> dict a, b1, sd, n_included, N, rounds, status"""
    hist = np.asarray(hist, dtype=np.float64).reshape(LBINS, SBINS)
    sumlen = np.asarray(sumlen, dtype=np.float64).reshape(LBINS)
    nb = hist.sum(axis=1)
    populated = nb > 0
    x = np.zeros(LBINS)
    x[populated] = np.log(sumlen[populated] / nb[populated])
    out = {"a": 0.0, "b1": 0.0, "sd": 0.0, "n_included": 0, "N": int(hist.sum()), "rounds": 0, "status": NO_FIT}
    eligible = np.zeros((LBINS, SBINS), dtype=bool)
    eligible[populated, 1:SBINS - 1] = True
    X = np.repeat(x[:, None], SBINS, axis=1)
    S = np.repeat(np.arange(SBINS, dtype=np.float64)[None, :], LBINS, axis=0)
    included = eligible.copy()
    for rounds in range(1, 11):
        w = np.where(included, hist, 0.0)
        n, sx, ss = w.sum(), (w * X).sum(), (w * S).sum()
        sxx, sxs = (w * X * X).sum(), (w * X * S).sum()
        out["rounds"], out["n_included"] = rounds, int(n)
        if n < 100:
            out["status"] = NO_FIT
            return out
        den = n * sxx - sx * sx
        b1 = 0.0 if den == 0 or included.any(axis=1).sum() < 2 else (n * sxs - sx * ss) / den
        a = (ss - b1 * sx) / n
        var = (w * (S - a - b1 * X) ** 2).sum() / (n - 2)
        out["a"], out["b1"] = float(a), float(b1)
        if not var > 0:
            out["sd"], out["status"] = 0.0, NO_FIT
            return out
        sd = float(np.sqrt(var))
        out["sd"], out["status"] = sd, OK
        z = (S - a - b1 * X) / sd
        nxt = eligible & (z >= -5) & (z <= 5)
        if (nxt == included).all():
            break
        included = nxt
    return out


def evalues(stats, scores, lengths):
    """-> (z, E) float64 arrays; NO_FIT: zeros and -1"""
    scores = np.asarray(scores, dtype=np.float64)
    lengths = np.maximum(np.asarray(lengths, dtype=np.float64), 1.0)
    if stats["status"] != OK:
        return np.zeros(len(scores)), -np.ones(len(scores))
    z = (scores - stats["a"] - stats["b1"] * np.log(lengths)) / stats["sd"]
    p = -np.expm1(-np.exp(-(np.pi / np.sqrt(6.0)) * z - EULER_GAMMA))
    return z, stats["N"] * p
