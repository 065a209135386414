"""An independent full-matrix Gotoh SCORE in int64 numpy, vectorised over a batch of jobs of one shape.

Written from the reference's definitions of the text-blocking full-matrix aligner (nvbio/alignment/gotoh/gotoh_inl.h), not from the
oracle: pattern symbols are the rows i = 0..M-1, text symbols the columns j = 0..N-1, and

    H(-1, -1) = 0
    H(-1, j)  = G_o + G_e * j            GLOBAL  (the first band, :1188: the first gap symbol costs G_o)      0 otherwise
    H(i, -1)  = T_o + T_e * i            GLOBAL and SEMI_GLOBAL (the column init, :84-86, text gap costs)    0 for LOCAL
    E(i, -1)  = 0 for LOCAL, the infimum otherwise;  F(-1, j) = the infimum;  infimum = -32768 - min(G_o, G_e)   (:1162)
    F(i, j)   = max(F(i-1, j) + G_e, H(i-1, j) + G_o)
    E(i, j)   = max(E(i, j-1) + G_e, H(i, j-1) + G_o)
    H(i, j)   = max(E, F, H(i-1, j-1) + S(i, j)),  clamped at 0 for LOCAL

with G_o / G_e the pattern gap costs and T_o / T_e the text gap costs (equal for a plain Gotoh scheme), S = match on equal symbols and
otherwise the mismatch (the quality scheme: the LUT entry of the pattern symbol's quality).  The score is H(M-1, N-1) for GLOBAL, the
largest H of the last row for SEMI_GLOBAL and the largest H of the matrix for LOCAL.  No int16 anywhere: the model equals the
reference wherever the reference's int16 boundary column cannot truncate.  Sinks are not modelled (their tie-breaks are the oracle's).
"""
import numpy as np

GLOBAL, LOCAL, SEMI_GLOBAL = 0, 1, 2


def gotoh_score(ty, match, go, ge, tgo, tge, pats, txts, sub_mismatch):
    """pats int[B, M] (symbols; anything that differs from the text's 0..3 is a mismatch), txts int[B, N], sub_mismatch int[B, M]:
    the mismatch score of each pattern symbol (a constant for the plain scheme, LUT[quality] for the quality scheme) -> int64[B]."""
    pats, txts = np.asarray(pats, np.int64), np.asarray(txts, np.int64)
    mm = np.asarray(sub_mismatch, np.int64)
    B, M = pats.shape
    N = txts.shape[1]
    assert M >= 1 and N >= 1 and mm.shape == (B, M)
    inf = -32768 - min(go, ge)
    cols = np.arange(N, dtype=np.int64)
    # the row above the matrix, H(-1, j), and the corner H(-1, -1)
    Hprev = np.broadcast_to(go + ge * cols if ty == GLOBAL else np.zeros(N, np.int64), (B, N)).copy()
    corner = np.zeros(B, np.int64)
    F = np.full((B, N), inf, np.int64)
    best = np.full(B, np.iinfo(np.int64).min, np.int64)
    for i in range(M):
        left = np.full(B, 0 if ty == LOCAL else tgo + tge * i, np.int64)              # H(i, -1)
        E = np.full(B, 0 if ty == LOCAL else inf, np.int64)                           # E(i, -1)
        F = np.maximum(F + ge, Hprev + go)
        S = np.where(txts == pats[:, i:i + 1], match, mm[:, i:i + 1])
        diag = np.concatenate([corner[:, None], Hprev[:, :-1]], axis=1) + S
        H = np.empty((B, N), np.int64)
        h = left
        for j in range(N):
            E = np.maximum(E + ge, h + go)
            h = np.maximum(np.maximum(E, F[:, j]), diag[:, j])
            if ty == LOCAL:
                h = np.maximum(h, 0)
            H[:, j] = h
        if ty == LOCAL:
            best = np.maximum(best, H.max(axis=1))
        corner = left
        Hprev = H
    if ty == GLOBAL:
        return Hprev[:, -1]
    if ty == SEMI_GLOBAL:
        return Hprev.max(axis=1)
    return best
