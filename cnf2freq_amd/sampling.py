"""Posterior sampling of inheritance paths (Context.sweep_sample, include/cnf2hip.h: cnf2_sweep_sample): the generator
the draws use, restated in numpy so that every pick can be replayed, and the order in which a pick lays out the states.
Crossover events of the draws: viterbi.crossover_calls(state.reshape(n * K, M), chromstarts)."""
import numpy as np

from . import synth

# The order in which the 64 states g = j*8 + lo are laid on [0, W) by every state pick: ascending (the kernel sums the
# weights of the groups j*8 .. j*8 + 7 first, then walks the states of the chosen group).  Modes are laid in ascending
# order too.
STATE_ORDER = np.arange(64)


def _mix(z):
    """SplitMix64's output function of z (mod 2^64)."""
    return synth.splitmix64(np.asarray(z, dtype=np.uint64), 0)


def keys(seed, ind, draw):
    """key(seed, i, k) = mix(mix(mix(seed) ^ i) ^ k), broadcast over the arguments (uint64)."""
    with np.errstate(over="ignore"):
        s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        return _mix(_mix(_mix(s) ^ np.asarray(ind, dtype=np.uint64)) ^ np.asarray(draw, dtype=np.uint64))


def uniforms(seed, ind, draw, j):
    """u(seed, i, k, j) in [0, 1): j = m for the state at marker m, j = n_markers + c for the mode on chromosome c.
    i is the absolute index of the analysed individual.  Broadcast over ind, draw and j."""
    k = keys(seed, ind, draw)
    return synth.uniform(k ^ np.asarray(j, dtype=np.uint64), 0)
