"""Reference of posterior decoding for the tests: fp64 class sums of a posterior tensor, the lowest maximal class per
position, that class's posterior, and the margin between the two best classes — the distance within which a rounding
error of the code under test may legitimately pick the other class."""
import numpy as np


def decode(gamma, state_class=None, C=None):
    """gamma (..., q) -> (label uint8 (...), conf fp64 (...), margin fp64 (...)).  state_class: q class indices in
    0..C-1, or None for the identity map (C = q).  margin is +inf with one class."""
    g = np.asarray(gamma, dtype=np.float64)
    q = g.shape[-1]
    if state_class is None:
        cls = g
    else:
        table = np.asarray(state_class, dtype=np.int64).reshape(-1)
        assert table.shape == (q,) and table.min() >= 0 and table.max() < C
        cls = np.zeros(g.shape[:-1] + (C,), dtype=np.float64)
        for s in range(q):                                        # states in increasing index
            cls[..., table[s]] += g[..., s]
    label = cls.argmax(-1)                                        # numpy: the first maximal index
    conf = np.take_along_axis(cls, label[..., None], -1)[..., 0]
    if cls.shape[-1] == 1:
        margin = np.full(conf.shape, np.inf)
    else:
        top2 = np.partition(cls, -2, axis=-1)
        margin = top2[..., -1] - top2[..., -2]
    return label.astype(np.uint8), conf, margin


# the 15-state gene model (Ir, I0-2, E0-2, START, EI0-2, IE0-2, STOP) onto intergenic / intron / exon phase 0, 1, 2;
# the largest class (the intron with its splice-site states) has n_max = 9 states
GENE_CLASSES = [0, 1, 1, 1, 2, 3, 4, 2, 1, 1, 1, 1, 1, 1, 4]
GENE_NMAX = 9


def random_map(rng, q, C, empty=None):
    """q class indices in 0..C-1 with every class used (as far as q allows), except `empty` (never used)."""
    use = [c for c in range(C) if c != empty]
    table = [use[i % len(use)] for i in range(q)]
    rng.shuffle(table)
    return [int(c) for c in table]
