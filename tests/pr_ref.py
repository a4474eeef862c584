"""Numpy restatement of place recognition (csrc/uvs_place_recognition.hip, the rule in include/uvs_solver.h): the vocabulary tree's descent, the
tf-idf bag-of-words vector, the L1 query of the database and detectLoop's gates, as the reference does them (pose_graph.cpp:304-386;
DBoW2's TemplatedVocabulary::transform, BowVector::addWeight / normalize, TemplatedDatabase::queryL1).  Every floating-point operation is an
FP64 add, subtract or divide in the reference's order (numpy's cumsum adds one element after the other), so the device is held to it bit for
bit.  A vocabulary is the dict of abi.load_vocabulary."""
import numpy as np


class Tree:
    """Per node id (0 = the root): children in the order of their records, descriptor, word id (-1: inner), weight."""

    def __init__(self, voc):
        nid = np.asarray(voc["node_id"], np.int64); pid = np.asarray(voc["parent_id"], np.int64)
        S = len(nid) + 1
        self.L = int(voc["L"])
        self.cnt = np.zeros(S, np.int64)
        kids = [[] for _ in range(S)]
        for n, p in zip(nid, pid):
            kids[p].append(int(n))
        self.cnt = np.array([len(c) for c in kids], np.int64)
        self.kmax = max(int(self.cnt.max()), 1)
        self.children = np.zeros((S, self.kmax), np.int64)
        for i, c in enumerate(kids):
            self.children[i, :len(c)] = c
        self.desc = np.zeros((S, 4), np.uint64); self.desc[nid] = np.asarray(voc["descriptor"], np.uint64).reshape(-1, 4)
        self.weight = np.zeros(S); self.weight[nid] = np.asarray(voc["weight"], np.float64)
        self.word = -np.ones(S, np.int64); self.word[np.asarray(voc["word_node_id"], np.int64)] = np.asarray(voc["word_id"], np.int64)


def hamming(a, b):
    """Bits that differ between uint64 [..., 4] descriptors."""
    return np.bitwise_count(np.bitwise_xor(a, b)).sum(axis=-1).astype(np.int64)


def transform(tree, desc):
    """desc uint64 [n, 4] -> (word id int32 [n], weight [n]): from the root to the child of the smallest distance, the first of equals, until a leaf."""
    desc = np.asarray(desc, np.uint64).reshape(-1, 4)
    node = np.zeros(len(desc), np.int64)
    rows = np.arange(len(desc))
    for _ in range(tree.L):
        cnt = tree.cnt[node]
        if not len(desc) or not (cnt > 0).any():
            break
        ch = tree.children[node]                                          # [n, kmax]
        d = hamming(tree.desc[ch], desc[:, None, :])
        d[np.arange(tree.kmax)[None, :] >= cnt[:, None]] = 1 << 20
        node = np.where(cnt > 0, ch[rows, np.argmin(d, axis=1)], node)     # argmin: the first minimum
    return tree.word[node].astype(np.int32), tree.weight[node].copy()


def bow(words, weights):
    """The keyframe's vector -> (word ids int32 ascending, values): stop words (weight <= 0) dropped, v = w then v += w per further
    occurrence, norm = the ordered sum of |v|, v / norm when norm > 0."""
    words = np.asarray(words, np.int64); weights = np.asarray(weights, np.float64)
    keep = weights > 0
    uw, first, count = np.unique(words[keep], return_index=True, return_counts=True)
    w = weights[keep][first]
    v = w.copy()
    for c in range(1, int(count.max()) if len(count) else 0):
        more = count > c
        v[more] = v[more] + w[more]
    norm = float(np.cumsum(np.abs(v))[-1]) if len(v) else 0.0
    if norm > 0.0:
        v = v / norm
    return uw.astype(np.int32), v


def vector(tree, desc):
    return bow(*transform(tree, desc))


def raw_score(q, d):
    """(s, common words): s = the ordered sum over the common words, ascending, of |q - d| - |q| - |d|."""
    _, iq, id_ = np.intersect1d(q[0], d[0], assume_unique=True, return_indices=True)
    if not len(iq):
        return 0.0, 0
    a, b = q[1][iq], d[1][id_]
    return float(np.cumsum(np.abs(a - b) - np.abs(a) - np.abs(b))[-1]), len(iq)


class Database:
    """Append-only; the entry id is the order of addition."""

    def __init__(self, tree):
        self.tree = tree
        self.entries = []

    def size(self):
        return len(self.entries)

    def clear(self):
        self.entries = []

    def add(self, desc):
        self.entries.append(vector(self.tree, desc))
        return len(self.entries) - 1

    def query_vector(self, q, max_results=4, max_id=-1):
        n = len(self.entries)
        res = []
        for e, d in enumerate(self.entries):
            if not (e < max_id or max_id == -1 or e == n - 1):
                continue
            s, hits = raw_score(q, d)
            if hits:
                res.append((s, e))
        res.sort()                                                         # ascending s, a tie to the lower id
        if max_results > 0:
            res = res[:max_results]
        return np.array([e for _, e in res], np.int32), np.array([-s / 2.0 for s, _ in res], np.float64)

    def query(self, desc, max_results=4, max_id=-1):
        return self.query_vector(vector(self.tree, desc), max_results, max_id)


def gates(ids, scores, frame_index):
    """detectLoop's decision on the query's results (pose_graph.cpp:348-385)."""
    find_loop = len(scores) >= 1 and scores[0] > 0.05 and any(s > 0.015 for s in scores[1:])
    if not (find_loop and frame_index > 50):
        return -1
    min_index = -1
    for i, s in zip(ids, scores):
        if min_index == -1 or (i < min_index and s > 0.015):
            min_index = int(i)
    return min_index


def detect(db, desc, frame_index):
    """-> (loop index or -1, ids, scores): query(4, frame_index - 50), then add, then the gates."""
    q = vector(db.tree, desc)
    ids, scores = db.query_vector(q, 4, frame_index - 50)
    db.entries.append(q)
    return gates(ids, scores, frame_index), ids, scores
