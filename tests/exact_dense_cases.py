"""The dense exact banks (tools/exact_bank.py: build_dense) that tests/test_gpu_exact_dense.py runs on
the device and tests/test_exact_dense_cpu.py first puts through the any-order float32 emulator.  A
bank enters a GPU test only through ``bank(name)``, so the two files cannot drift apart."""
import functools

from tools import exact_bank as X

K = 48                      # the default grades: weights 1 and 2^-3, l = 2
K_SHARP = 64                # tau = 44.36 > 43: the running-maximum pass 1; weights 1 and 2^-4

BANKS = {
    # k = 48, keys with mantissa perturbation: the sizes cross the 16-row block and several tiles
    "n9": dict(n=9, k=K, seed=9), "n16": dict(n=16, k=K, seed=16), "n17": dict(n=17, k=K, seed=17),
    "n108": dict(n=108, k=K, seed=108), "n1537": dict(n=1537, k=K, seed=1537), "n4099": dict(n=4099, k=K, seed=4099),
    # plain +-1/16 keys: what fp16 / bf16 hold, and what a bank file's float32 normalisation leaves alone
    "n108_plain": dict(n=108, k=K, seed=1108, perturb=False), "n4099_plain": dict(n=4099, k=K, seed=5099, perturb=False),
    # three grades (weights 2^-3 and 2^-6, l = 4/8 + 32/64 = 1: the value grid admits beta = 1 only)
    "g108": dict(n=108, k=K, seed=3108, classes=[(0, 4, 32)] * 3),
    "g1537": dict(n=1537, k=K, seed=4537, classes=[(0, 4, 32)] * 42 + [(8,), (8,), (8,), (1,)]),
    # graded geographic classes: one row at the axis, eight at 15/16 of it (l_geo = 2)
    "n108_geo": dict(n=108, k=K, seed=2108, geo_graded=True), "n1537_geo": dict(n=1537, k=K, seed=3537, geo_graded=True),
    # k = 64: classes 0, 1 (, 2) without a d = 0 row (the maximum is a graded row's); the d = 0 rows last
    "s108": dict(n=108, k=K_SHARP, seed=64),
    "s108_notop": dict(n=108, k=K_SHARP, seed=65, classes=X.dense_classes(108, K_SHARP, no_top=2)),
    "s108_last": dict(n=108, k=K_SHARP, seed=66, top_last=True),
    "s1537_last": dict(n=1537, k=K_SHARP, seed=67, classes=X.dense_classes(1537, K_SHARP, no_top=3), top_last=True),
}
NO_TOP = {"s108_notop": 2, "s1537_last": 3}      # the first classes of these banks hold no d = 0 row


@functools.lru_cache(maxsize=None)
def bank(name):
    return X.build_dense(**BANKS[name])


def perturbed(name) -> bool:
    return BANKS[name].get("perturb", True)


def tau(name) -> float:
    return X.dense_tau(BANKS[name]["k"])


def betas(name):
    """The blend weights the bank's value grid admits (X.dense_betas: from its classes' l and smallest
    weights - a term of weight 2^-4 / 2 at beta in quarters would leave the 2^-23 grid)."""
    return X.dense_betas(bank(name))


# stats_kept: the (k_sem, k_geo) pairs swept from one kept scan at k = 48 (0: no geographic head), B = 65
STATS_B = 65
STATS_PAIRS = {"n17": [(48, 48), (32, 32), (64, 64), (32, 64), (64, 48)],
               "n108": [(48, 48), (64, 64), (48, 64), (64, 0)]}


def stats_queries(name):
    return X.queries(bank(name), STATS_B, seed=STATS_B, perturb=True)


def pair_taus(pair):
    return tuple(X.dense_tau(k) if k else 0.0 for k in pair)


# load_model: (bank, as a prepared bank file) - an .npz bank's reader divides the keys by their float32
# norm, which only plain keys survive; a prepared file uploads perturbed keys and graded locations as
# they are.  The query is the plain direction of one class (a constant-bias encoder).
FORWARD_BANKS = [("n108_plain", False), ("n108", True), ("n108_geo", True)]
FORWARD_B = (5, 16, 17, 32, 65)      # attend_small_kernel + small_finalize_kernel up to 32, two passes above


def forward_class(name) -> int:
    """The first graded class (nine rows) on an odd Hadamard row: h[i] h[i ^ 1] = -1 there, so a kernel
    that pairs q[i] with k[i ^ 1] changes the similarity of even a plain query and a plain key."""
    b = bank(name)
    row = 1 + b.sem_dir % (X.KEY_DIM - 1)
    return int(next(c for c in range(b.n_classes) if b.sem_size[c] == 9 and row[c] & 1))
