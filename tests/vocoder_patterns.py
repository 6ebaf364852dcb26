"""GRU_A recurrent matrices with an explicit block pattern, for the tests of the vocoder's packing edges
(tests/test_gpu_vocoder_edges.py on the device, tests/test_vocoder_second_opinion.py on the CPU).

synth.lpcnet_weights prunes an i.i.d. matrix by a density, so the widths of its row groups are whatever the draw gives.
Here every one of the 3 x 48 row groups (8 outputs of one gate) keeps a stated set of its 96 column blocks (4 inputs
each): a count (the blocks of highest energy, as magnitude pruning keeps them) or a list of block indices.  The diagonal is
always kept; it is not part of any block (fpc_lpcnet_create and the oracle carry it separately).

`expectation` states what the widths imply for the library, by the arithmetic of csrc/lpcnet.hip's comments only: a group
of k blocks takes max(1, ceil(k / 4)) mat-vec lanes, the kernel instance follows the widest group of the update / reset
gates and of the candidate gate (rounded up to a power of two), two utterances per workgroup need every group padded to an
even number of lanes and no more than 512 lanes in all.  It does not place anything."""
import numpy as np

N, ROWS, COLS = 384, 48, 96   # units, block rows per gate (8 outputs), column blocks (4 inputs)


def _energy(rec, gate):
    """[48][96] off-diagonal energy of the 8x4 blocks of one gate (rows = outputs), as synth.lpcnet_weights ranks them"""
    A = rec[:, gate * N:(gate + 1) * N].astype(np.float64).copy()   # (in, out)
    np.fill_diagonal(A, 0)
    blk = A.T.reshape(ROWS, 8, COLS, 4)
    return (blk * blk).sum(axis=(1, 3))


def weights(synth, keep, scale=1.0, zero_diagonal=False):
    """the default weight set with gru_a_recurrent rebuilt: keep[gate][block row] = a count or a list of column blocks;
    the kept off-diagonal values are multiplied by `scale`.  Returns (weights, counts[3][48])."""
    w = synth.lpcnet_weights(density=(1.0, 1.0, 1.0))   # this mask keeps every block: the dense matrix
    rec = w["gru_a_recurrent"]
    out = np.zeros_like(rec)
    counts = np.zeros((3, ROWS), np.int64)
    for g in range(3):
        en = _energy(rec, g)
        mask = np.zeros((ROWS, COLS), bool)
        for rb in range(ROWS):
            k = keep[g][rb]
            cols = np.argsort(-en[rb], kind="stable")[:int(k)] if np.isscalar(k) else np.asarray(list(k), np.int64)
            mask[rb, cols] = True
            counts[g, rb] = len(cols)
        full = np.repeat(np.repeat(mask, 8, axis=0), 4, axis=1)           # (out, in)
        A = rec[:, g * N:(g + 1) * N] * full.T * np.float32(scale)
        A[np.arange(N), np.arange(N)] = 0.0 if zero_diagonal else np.diag(rec[:, g * N:(g + 1) * N])
        out[:, g * N:(g + 1) * N] = A
    w["gru_a_recurrent"] = np.ascontiguousarray(out.astype(np.float32))
    return w, counts


def _uniform(zr, n=None):
    return [[zr] * ROWS, [zr] * ROWS, [zr if n is None else n] * ROWS]


def _with(base, *edits):
    keep = [list(row) for row in base]
    for gate, rb, k in edits:
        keep[gate][rb] = k
    return keep


def skewed_counts(seed=2024, sigma=0.5, density=(0.05, 0.05, 0.2)):
    """blocks kept per block row drawn lognormal and scaled to the benchmark's mean densities: the skewed occupancy of a
    trained, magnitude-pruned matrix"""
    rng = np.random.default_rng(seed)
    keep = []
    for d in density:
        raw = rng.lognormal(0.0, sigma, ROWS)
        keep.append([int(k) for k in np.clip(np.rint(raw * (d * COLS / raw.mean())), 0, 64)])
    return keep


# name -> (keep, zero_diagonal).  Gate 0 = update (z), 1 = reset (r), 2 = candidate (n)
PATTERNS = {
    # 0..8 blocks in z and r, 0..32 in n: empty groups, lanes filled exactly and partly, odd lane counts
    "ladder": ([[rb % 9 for rb in range(ROWS)], [rb % 9 for rb in range(ROWS)], [(7 * rb) % 33 for rb in range(ROWS)]], False),
    # exactly the two blocks that hold the diagonal elements (in == o) of the block row
    "diagonal_crossing": ([[[2 * rb, 2 * rb + 1] for rb in range(ROWS)]] * 3, False),
    "diagonal_crossing_zero_diagonal": ([[[2 * rb, 2 * rb + 1] for rb in range(ROWS)]] * 3, True),
    "diagonal_only": (_uniform(0), False),
    # the widest groups instance 408 serves: 16 blocks = 4 lanes (z, r), 32 blocks = 8 lanes (n)
    "edge_of_408": (_with(_uniform(2), (0, 5, 16), (1, 17, 16), (2, 29, 32)), False),
    "one_past_the_edge_z17": (_with(_uniform(2), (0, 5, 17), (1, 17, 16), (2, 29, 32)), False),
    "one_past_the_edge_n33": (_with(_uniform(2), (0, 5, 16), (1, 17, 16), (2, 29, 33)), False),
    "widest_group": (_with(_uniform(2), (1, 40, 64)), False),     # 16 lanes: one whole DPP row
    # 144 groups of 3 lanes = 432 lanes fit; padded to 4 lanes they are 576 > 512
    "no_room_for_padding": (_uniform(9), False),
    "skewed": (skewed_counts(), False),
}
TOO_WIDE = _with(_uniform(2), (1, 40, 65))   # 17 lanes: refused


def build(synth, name, scale=1.0):
    keep, zero_diagonal = PATTERNS[name]
    return weights(synth, keep, scale=scale, zero_diagonal=zero_diagonal)


def expectation(counts):
    """(kernel instance, two utterances per workgroup possible) implied by the group widths"""
    lanes = np.maximum(1, -(-np.asarray(counts) // 4))
    pow2 = lambda q: 1 << int(q - 1).bit_length()
    qzr, qn = pow2(lanes[:2].max()), pow2(lanes[2].max())
    variant = 208 if qzr <= 2 and qn <= 8 else 408 if qzr <= 4 and qn <= 8 else 1616
    padded = int(((lanes + 1) // 2 * 2).sum())
    return variant, variant != 1616 and padded <= 512
