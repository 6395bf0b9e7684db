"""Crossover calls from decoded Viterbi paths (Context.sweep_viterbi)."""
import numpy as np


def crossover_calls(state, chromstarts):
    """One row (individual, chromosome, marker m, meiosis t) for every state bit t that flips between markers m and m+1
    of the same chromosome in the MAP paths state[n][M] (uint8).  Individuals skipped on a chromosome (0xFF) have none.
    Rows are ordered by individual, chromosome, marker, meiosis; int64 array of shape (k, 4)."""
    state = np.asarray(state, dtype=np.uint8)
    cs = np.asarray(chromstarts, dtype=np.int64)
    rows = []
    for c in range(len(cs) - 1):
        a, b = int(cs[c]), int(cs[c + 1])
        if b - a < 2:
            continue
        s = state[:, a:b].astype(np.int64)
        ok = (s[:, :-1] != 0xFF) & (s[:, 1:] != 0xFF)
        flip = (s[:, :-1] ^ s[:, 1:]) & np.where(ok, 63, 0)
        bits = (flip[..., None] >> np.arange(6)) & 1          # [n][gaps][6]
        i, g, t = np.nonzero(bits)
        rows.append(np.stack([i, np.full_like(i, c), a + g, t], axis=1))
    if not rows:
        return np.zeros((0, 4), np.int64)
    out = np.concatenate(rows)
    return out[np.lexsort((out[:, 3], out[:, 2], out[:, 1], out[:, 0]))]
