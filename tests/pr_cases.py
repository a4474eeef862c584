"""Cases for the tests of uvs_pr_* (csrc/uvs_place_recognition.hip): crafted vocabulary trees, a seeded vocabulary builder in DBoW2's manner
(hierarchical k-medians with majority-bit centres, idf weights over a training set of images) and the keyframe stream of lc_cases' MH_05
world.  Everything comes from seeds; nothing is stored."""
import functools

import numpy as np

import lc_cases
import pr_ref


def tree_from_parents(parents, desc, weights, k, L):
    """A vocabulary dict from parent ids (node i + 1 has parent parents[i]), records in id order, words given to the leaves in id order."""
    parents = np.asarray(parents, np.int32)
    n = len(parents)
    ids = np.arange(1, n + 1, dtype=np.int32)
    leaf = ~np.isin(ids, parents)
    return dict(k=k, L=L, scoring=0, weighting=0, node_id=ids, parent_id=parents, weight=np.asarray(weights, np.float64).copy(),
                descriptor=np.asarray(desc, np.uint64).reshape(n, 4).copy(), word_node_id=ids[leaf].copy(), word_id=np.arange(leaf.sum(), dtype=np.int32))


def full_tree(seed, k, L, stop_every=0):
    """A full k-ary tree of depth L with random centres and weights in (0.5, 3); every stop_every-th word has weight 0."""
    rng = np.random.default_rng(seed)
    parents, level = [], [0]
    for _ in range(L):
        nxt = []
        for p in level:
            for _ in range(k):
                parents.append(p); nxt.append(len(parents))
        level = nxt
    n = len(parents)
    w = rng.uniform(0.5, 3.0, n)
    voc = tree_from_parents(parents, lc_cases.random_desc(rng, n), w, k, L)
    if stop_every:
        stop = voc["word_node_id"][voc["word_id"] % stop_every == 0]
        voc["weight"][stop - 1] = 0.0
    return voc


def unbalanced_tree(seed=3):
    """Leaves at depths 1, 2 and 3 (L = 3): 1 leaf, 2 inner -> (3 leaf, 4 inner -> (6, 7, 8 leaves), 5 leaf)."""
    rng = np.random.default_rng(seed)
    parents = [0, 0, 2, 2, 2, 4, 4, 4]
    return tree_from_parents(parents, lc_cases.random_desc(rng, 8), rng.uniform(0.5, 3.0, 8), 3, 3)


def shuffled(voc, seed=4):
    """The same tree with its ids relabelled at random and its records in another order (siblings keep their relative order, so the
    relabelled tree maps every descriptor to the same word); child ids are then neither contiguous nor ascending."""
    rng = np.random.default_rng(seed)
    n = len(voc["node_id"])
    relabel = np.r_[0, rng.permutation(n) + 1].astype(np.int32)           # old id -> new id
    order = rng.permutation(n)
    # keep siblings in their relative order: sort the shuffled record positions within every parent
    by_parent = {}
    for pos in np.sort(order):
        by_parent.setdefault(int(voc["parent_id"][pos]), []).append(pos)
    slots = {p: sorted(np.flatnonzero(np.isin(order, v))) for p, v in by_parent.items()}
    new_order = order.copy()
    for p, v in by_parent.items():
        new_order[slots[p]] = v
    out = dict(voc)
    out["node_id"] = relabel[voc["node_id"][new_order]]; out["parent_id"] = relabel[voc["parent_id"][new_order]]
    out["weight"] = voc["weight"][new_order].copy(); out["descriptor"] = voc["descriptor"][new_order].copy()
    wperm = rng.permutation(len(voc["word_id"]))
    out["word_node_id"] = relabel[voc["word_node_id"][wperm]]; out["word_id"] = voc["word_id"][wperm].copy()
    return out


def tie_tree():
    """k = 3, L = 2.  The root's children 1 and 2 are both at distance 1 from TIE_QUERY (child 3 is far), and under each of them the
    children 1 and 2 of three are IDENTICAL, so every step of the descent of TIE_QUERY is a tie that the earlier child wins."""
    d = np.zeros((12, 4), np.uint64)
    d[1, 0] = 3                        # node 2: bits 0 and 1;   node 1: no bit;   the query: bit 0
    d[2] = np.uint64(2 ** 64 - 1)      # node 3: far
    for base in (3, 6, 9):             # children of nodes 1, 2, 3: two identical, one far
        d[base] = d[base + 1] = (5, 0, 0, 0)
        d[base + 2] = np.uint64(2 ** 64 - 1)
    parents = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    return tree_from_parents(parents, d, np.arange(1, 13) * 0.25, 3, 2)


TIE_QUERY = np.array([[1, 0, 0, 0]], np.uint64)
TIE_WORD = 0                           # node 4 = the first child of node 1 = the first leaf


def crafted():
    """name -> vocabulary."""
    return {"k3L2": full_tree(1, 3, 2), "k10L3": full_tree(2, 10, 3), "unbalanced": unbalanced_tree(), "shuffled": shuffled(full_tree(1, 3, 2)),
            "tie": tie_tree(), "stop": full_tree(5, 4, 2, stop_every=3)}


def descriptors_near(voc, seed, n, p=0.1):
    """n descriptors: centres of the vocabulary's leaves with a share p of their bits flipped (so that words repeat within a frame)."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 4), np.uint64)
    leaves = np.asarray(voc["word_node_id"]) - 1
    rec = np.argsort(voc["node_id"])                                       # node id - 1 -> record
    pick = rec[leaves[rng.integers(0, len(leaves), n)]]
    return lc_cases.flip_bits(rng, voc["descriptor"][pick], p=p)


# ---------------------------------------------------------------- the seeded builder
def _bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc).view(np.uint8), axis=1, bitorder="little")


def _pack(bits):
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(-1, 4)


def build_vocabulary(desc, images, k, L, seed=0, iterations=4):
    """Hierarchical k-medians over desc uint64 [n, 4] (centres: the majority of every bit, a tie to 0), at most L levels; a cluster of at most
    k descriptors becomes that many leaves.  images: list of index arrays into desc; weight = log(N / N_i) with N_i the images that hold the
    word, 0 for a word no image holds."""
    rng = np.random.default_rng(seed)
    desc = np.asarray(desc, np.uint64).reshape(-1, 4)
    bits = _bits(desc)
    parents, centres = [], []

    def split(idx, parent, depth):
        if len(idx) <= k:
            groups = [idx[i:i + 1] for i in range(len(idx))]
            cs = desc[idx]
        else:
            cs = desc[rng.choice(idx, k, replace=False)]
            for _ in range(iterations):
                assign = np.argmin(pr_ref.hamming(cs[None, :, :], desc[idx][:, None, :]), axis=1)
                groups = [idx[assign == c] for c in range(len(cs))]
                groups = [g for g in groups if len(g)]
                cs = _pack(np.stack([(2 * bits[g].sum(axis=0) > len(g)).astype(np.uint8) for g in groups]))
            assign = np.argmin(pr_ref.hamming(cs[None, :, :], desc[idx][:, None, :]), axis=1)
            keep = [c for c in range(len(cs)) if (assign == c).any()]
            groups = [idx[assign == c] for c in keep]; cs = cs[keep]
        made = []
        for c in range(len(groups)):
            parents.append(parent); centres.append(cs[c]); made.append(len(parents))
        for node, g in zip(made, groups):
            if depth + 1 < L and len(g) > 1:
                split(g, node, depth + 1)

    split(np.arange(len(desc)), 0, 0)
    voc = tree_from_parents(parents, np.array(centres, np.uint64), np.zeros(len(parents)), k, L)
    tree = pr_ref.Tree(voc)
    words, _ = pr_ref.transform(tree, desc)
    n_i = np.zeros(len(voc["word_id"]))
    for im in images:
        n_i[np.unique(words[im])] += 1
    with np.errstate(divide="ignore"):
        w = np.where(n_i > 0, np.log(len(images) / np.maximum(n_i, 1)), 0.0)
    voc["weight"][voc["word_node_id"] - 1] = w[voc["word_id"]]
    return voc


# ---------------------------------------------------------------- MH_05
MH05_K, MH05_L = 10, 5


@functools.lru_cache(maxsize=1)
def mh05():
    """-> dict(world, voc, tree, desc [k] = the keypoint descriptors of keyframe k).  The vocabulary is trained on the world's landmark
    descriptors (recovered as the bitwise majority of every landmark's observations; the images of the idf weights are the keyframes)."""
    world = lc_cases.mh05_world()
    n_lm = world["vis"].shape[1]
    acc = np.zeros((n_lm, 256), np.int32); seen = np.zeros(n_lm, np.int32)
    for k, kf in enumerate(world["kf"]):
        ids = world["keypts"][k]; m = ids >= 0
        np.add.at(acc, ids[m], _bits(kf["odesc"][m])); np.add.at(seen, ids[m], 1)
    lm = np.flatnonzero(seen > 0)
    ldesc = _pack((2 * acc[lm] > seen[lm, None]).astype(np.uint8))
    row = -np.ones(n_lm, int); row[lm] = np.arange(len(lm))
    images = [row[np.unique(world["keypts"][k][world["keypts"][k] >= 0])] for k in range(len(world["kf"]))]
    voc = build_vocabulary(ldesc, images, MH05_K, MH05_L, seed=7)
    return dict(world=world, voc=voc, tree=pr_ref.Tree(voc), desc=[kf["odesc"] for kf in world["kf"]])


@functools.lru_cache(maxsize=1)
def mh05_detections():
    """pr_ref.detect over the stream, frame_index = the keyframe's number -> list of (loop index, ids, scores)."""
    m = mh05()
    db = pr_ref.Database(m["tree"])
    return [pr_ref.detect(db, d, k) for k, d in enumerate(m["desc"])]
