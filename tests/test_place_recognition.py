"""Place recognition (uvs_pr_*, csrc/uvs_place_recognition.hip): the vocabulary file, the host-only vocabulary check, the numpy restatement
tests/pr_ref.py against literal replays of the reference's rule, and the device against pr_ref bit for bit."""
import ctypes as C
import importlib
import os
import struct

import numpy as np
import pytest

import lc_cases as lc
import pg_ref
import pr_cases
import pr_ref

uvs = importlib.import_module("uv-slam_amd")
abi = uvs.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so")
PR_SYMBOLS = ["uvs_pr_check_vocabulary", "uvs_pr_create", "uvs_pr_destroy", "uvs_pr_last_error", "uvs_pr_size", "uvs_pr_clear", "uvs_pr_transform",
              "uvs_pr_add", "uvs_pr_query", "uvs_pr_detect", "uvs_pr_last_device_ms"]
# the MH_05 stream through pr_ref.detect (recorded from this CPU run): 20 revisiting keyframes get a candidate within
# lc.mh05_candidates' radius; 152 of the 223 keyframes get one farther away (the world is one room: keyframes metres apart share landmarks,
# and detectLoop returns the OLDEST of its results)
MH05_NEAR_RECORDED, MH05_FAR_RECORDED = 20, 152
RADIUS = 0.7


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------- the vocabulary file
def test_vocabulary_file_round_trip_and_layout(tmp_path):
    voc = pr_cases.crafted()["unbalanced"]
    p = str(tmp_path / "voc.bin"); p2 = str(tmp_path / "voc2.bin")
    abi.save_vocabulary(p, voc)
    raw = open(p, "rb").read()
    nn, nw = len(voc["node_id"]), len(voc["word_id"])
    assert len(raw) == 24 + 48 * nn + 8 * nw
    assert struct.unpack_from("<6i", raw, 0) == (voc["k"], voc["L"], 0, 0, nn, nw)
    for i in (0, nn - 1):
        rec = struct.unpack_from("<iid4Q", raw, 24 + 48 * i)
        assert rec[:2] == (voc["node_id"][i], voc["parent_id"][i]) and rec[2] == voc["weight"][i] and rec[3:] == tuple(int(x) for x in voc["descriptor"][i])
    assert struct.unpack_from("<ii", raw, 24 + 48 * nn + 8 * (nw - 1)) == (voc["word_node_id"][-1], voc["word_id"][-1])
    back = abi.load_vocabulary(p)
    for k in ("k", "L", "scoring", "weighting"):
        assert back[k] == voc[k]
    for k in ("node_id", "parent_id", "descriptor", "word_node_id", "word_id"):
        assert np.array_equal(back[k], voc[k]), k
    assert bits_equal(back["weight"], voc["weight"])
    abi.save_vocabulary(p2, back)
    assert open(p2, "rb").read() == raw
    open(p2, "wb").write(raw[:-3])
    with pytest.raises(ValueError):
        abi.load_vocabulary(p2)


# ---------------------------------------------------------------- the host-only check
def test_check_vocabulary_accepts_the_crafted_trees():
    for name, voc in pr_cases.crafted().items():
        assert uvs.api.check_vocabulary(voc) == (abi.UVS_OK, ""), name


def _malformed():
    base = pr_cases.full_tree(1, 3, 2)                     # nodes 1..3 under the root, 4..12 the leaves, words 0..8

    def edit(**kw):
        v = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in base.items()}
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v

    out = {"id_out_of_range": (edit(node_id=(0, 13)), "outside"), "id_below_range": (edit(node_id=(0, 0)), "outside"),
           "id_twice": (edit(node_id=(0, 2)), "twice"), "no_such_parent": (edit(parent_id=(5, 40)), "parent"),
           "negative_parent": (edit(parent_id=(5, -1)), "parent"), "negative_weight": (edit(weight=(2, -0.5)), "weight"),
           "nan_weight": (edit(weight=(7, np.nan)), "weight"), "inf_weight": (edit(weight=(7, np.inf)), "weight")}
    v = edit(); v["parent_id"][3] = 5; v["parent_id"][4] = 4             # nodes 4 and 5 are each other's parent
    out["cycle"] = (v, "cycle")
    v = edit(); v["parent_id"][3] = 4                                    # node 4 is its own parent
    out["self_parent"] = (v, "cycle")
    v = edit(); v["L"] = 1
    out["deeper_than_L"] = (v, "deeper")
    wide = pr_cases.tree_from_parents([0] * 17, lc.random_desc(np.random.default_rng(0), 17), np.ones(17), 10, 1)
    out["too_many_children"] = (wide, "children")
    v = edit(); v["word_node_id"] = v["word_node_id"][:-1]; v["word_id"] = v["word_id"][:-1]
    out["leaf_without_word"] = (v, "no word")
    v = edit(); v["word_node_id"] = np.r_[v["word_node_id"], 1].astype(np.int32); v["word_id"] = np.r_[v["word_id"], 9].astype(np.int32)
    out["word_on_inner_node"] = (v, "inner")
    v = edit(word_id=(3, 4))
    out["word_id_twice"] = (v, "twice")
    v = edit(word_id=(3, 9))
    out["word_id_out_of_range"] = (v, "outside")
    v = edit(); v["parent_id"][:3] = (2, 3, 1)                           # nothing hangs under the root (and 1 -> 2 -> 3 -> 1)
    out["root_without_children"] = (v, "root")
    empty = dict(base, node_id=np.zeros(0, np.int32), parent_id=np.zeros(0, np.int32), weight=np.zeros(0), descriptor=np.zeros((0, 4), np.uint64),
                 word_node_id=np.zeros(0, np.int32), word_id=np.zeros(0, np.int32))
    out["no_nodes"] = (empty, "root")
    return out


@pytest.mark.parametrize("name", sorted(_malformed()))
def test_check_vocabulary_rejects(name):
    voc, word = _malformed()[name]
    rc, msg = uvs.api.check_vocabulary(voc)
    assert rc == abi.UVS_ERR_INVALID_ARG and word in msg, (name, rc, msg)


def test_check_vocabulary_builds_tf_idf_l1_only():
    base = pr_cases.full_tree(1, 3, 2)
    assert uvs.api.check_vocabulary(dict(base, scoring=1))[0] == abi.UVS_ERR_UNSUPPORTED
    assert uvs.api.check_vocabulary(dict(base, weighting=1))[0] == abi.UVS_ERR_UNSUPPORTED


def test_pr_symbols_and_abi_version():
    L = uvs.api.lib()
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    assert "#define UVS_ABI_VERSION 7" in hdr and L.uvs_abi_version() == 7
    for s in PR_SYMBOLS:
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(L, s), s
    assert f"#define UVS_PR_MAX_K {abi.PR_MAX_K}" in hdr and f"#define UVS_PR_DETECT_RESULTS {abi.PR_DETECT_RESULTS}" in hdr
    assert f"#define UVS_PR_MAX_FRAMES {abi.PR_MAX_FRAMES}" in hdr and f"#define UVS_PR_MAX_L {abi.PR_MAX_L}" in hdr
    assert hasattr(C.CDLL(HOST), "uvs_host_pose_graph_detect_run")


# ---------------------------------------------------------------- pr_ref against literal replays
def _scalar_transform(voc, d):
    """TemplatedVocabulary::transform for one descriptor: plain loops over the file's records."""
    kids = {}
    for n, p in zip(voc["node_id"], voc["parent_id"]):
        kids.setdefault(int(p), []).append(int(n))
    rec = {int(n): i for i, n in enumerate(voc["node_id"])}
    word = {int(n): int(w) for n, w in zip(voc["word_node_id"], voc["word_id"])}
    node = 0
    while kids.get(node):
        best, best_d = None, None
        for c in kids[node]:
            dist = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(voc["descriptor"][rec[c]], d))
            if best is None or dist < best_d:              # strict: the earlier child keeps a tie
                best, best_d = c, dist
        node = best
    return word[node], float(voc["weight"][rec[node]])


@pytest.mark.parametrize("name", sorted(pr_cases.crafted()))
def test_ref_transform_is_the_scalar_descent(name):
    voc = pr_cases.crafted()[name]
    tree = pr_ref.Tree(voc)
    desc = np.r_[pr_cases.descriptors_near(voc, 11, 40), lc.random_desc(np.random.default_rng(12), 20)]
    words, weights = pr_ref.transform(tree, desc)
    for i, d in enumerate(desc):
        assert (int(words[i]), float(weights[i])) == _scalar_transform(voc, d), i


def test_ref_tie_goes_to_the_earlier_child():
    voc = pr_cases.tie_tree()
    words, weights = pr_ref.transform(pr_ref.Tree(voc), pr_cases.TIE_QUERY)
    assert words[0] == pr_cases.TIE_WORD and weights[0] == 1.0          # node 4: weight 4 * 0.25
    assert _scalar_transform(voc, pr_cases.TIE_QUERY[0])[0] == pr_cases.TIE_WORD
    sw, _ = pr_ref.transform(pr_ref.Tree(pr_cases.shuffled(voc)), pr_cases.TIE_QUERY)
    assert sw[0] == pr_cases.TIE_WORD


def test_ref_shuffled_records_give_the_same_words():
    a, b = pr_cases.crafted()["k3L2"], pr_cases.crafted()["shuffled"]
    assert not np.array_equal(a["node_id"], b["node_id"])
    desc = pr_cases.descriptors_near(a, 13, 200)
    wa, xa = pr_ref.transform(pr_ref.Tree(a), desc); wb, xb = pr_ref.transform(pr_ref.Tree(b), desc)
    assert np.array_equal(wa, wb) and bits_equal(xa, xb)


def _dict_bow(words, weights):
    """BowVector::addWeight per feature, then normalize(L1): a literal replay."""
    v = {}
    for w, x in zip(words, weights):
        if x > 0:
            if int(w) in v:
                v[int(w)] += float(x)
            else:
                v[int(w)] = float(x)
    norm = 0.0
    for w in sorted(v):
        norm += abs(v[w])
    if norm > 0.0:
        for w in v:
            v[w] /= norm
    ks = sorted(v)
    return np.array(ks, np.int32), np.array([v[k] for k in ks], np.float64)


@pytest.mark.parametrize("name,n", [("k3L2", 700), ("stop", 300), ("k10L3", 500), ("unbalanced", 90)])
def test_ref_bow_is_the_map_replay(name, n):
    voc = pr_cases.crafted()[name]
    words, weights = pr_ref.transform(pr_ref.Tree(voc), pr_cases.descriptors_near(voc, 14, n))
    bw, bv = pr_ref.bow(words, weights)
    dw, dv = _dict_bow(words, weights)
    assert np.array_equal(bw, dw) and bits_equal(bv, dv)
    assert np.all(np.diff(bw) > 0) and abs(bv.sum() - 1.0) < 1e-12
    if name == "stop":
        assert (weights == 0).any() and not np.isin(words[weights == 0], bw).any()
    if name == "k3L2":
        assert np.bincount(words).max() > 50                             # long runs of repeated adds


def test_ref_bow_of_nothing_and_of_stop_words_only():
    assert len(pr_ref.bow(np.zeros(0, np.int32), np.zeros(0))[0]) == 0
    assert len(pr_ref.bow(np.array([3, 3, 5]), np.zeros(3))[0]) == 0


def test_ref_score_is_one_minus_half_the_l1_distance():
    voc = pr_cases.crafted()["k10L3"]
    tree = pr_ref.Tree(voc)
    db = pr_ref.Database(tree)
    for f in range(12):
        db.add(pr_cases.descriptors_near(voc, 100 + f, 150 + 10 * f))
    q = pr_ref.vector(tree, pr_cases.descriptors_near(voc, 99, 220))
    ids, scores = db.query_vector(q, 0, -1)
    assert len(ids) == 12
    dense_q = np.zeros(len(voc["word_id"]), np.longdouble); dense_q[q[0]] = q[1]
    for e, s in zip(ids, scores):
        dense_d = np.zeros(len(voc["word_id"]), np.longdouble); dense_d[db.entries[e][0]] = db.entries[e][1]
        want = np.longdouble(1) - np.longdouble(0.5) * np.abs(dense_q - dense_d).sum()
        assert abs(np.longdouble(s) - want) <= 4 * np.finfo(np.float64).eps, (e, s, want)
    assert np.all(np.diff(scores) <= 0)


def _vec(words, values):
    return np.array(words, np.int32), np.array(values, np.float64)


def test_ref_three_entry_example_by_hand():
    db = pr_ref.Database(None)
    db.entries = [_vec([1], [1.0]),                    # |0.5 - 1| - 0.5 - 1 = -1                 -> Score 0.5
                  _vec([2, 3], [0.5, 0.5]),            # 2 x (|0.25 - 0.5| - 0.25 - 0.5) = -1      -> Score 0.5: the tie goes to entry 0
                  _vec([4, 9], [0.5, 0.5]),            # no common word: no result
                  _vec([1, 2, 3], [0.5, 0.25, 0.25])]  # the query itself: -1 - 0.5 - 0.5 = -2     -> Score 1
    q = _vec([1, 2, 3], [0.5, 0.25, 0.25])
    ids, scores = db.query_vector(q, 0, -1)
    assert ids.tolist() == [3, 0, 1] and scores.tolist() == [1.0, 0.5, 0.5]
    ids, scores = db.query_vector(q, 2, -1)
    assert ids.tolist() == [3, 0] and scores.tolist() == [1.0, 0.5]
    # eligibility: e < max_id || max_id == -1 || e == n - 1
    assert db.query_vector(q, 0, -2)[0].tolist() == [3]                  # below -1: the last entry only
    assert db.query_vector(q, 0, 0)[0].tolist() == [3]
    assert db.query_vector(q, 0, 1)[0].tolist() == [3, 0]
    assert db.query_vector(q, 0, 3)[0].tolist() == [3, 0, 1]             # n - 1: everything below the last, and the last anyway
    db.entries.append(_vec([7], [1.0]))                                   # now the last entry shares no word: eligible, but no result
    assert db.query_vector(q, 0, 0)[0].tolist() == []
    assert db.query_vector(q, 0, -1)[0].tolist() == [3, 0, 1]
    assert db.query_vector(_vec([], []), 0, -1)[0].tolist() == []


def test_ref_detect_gates_at_their_edges():
    g = pr_ref.gates
    assert g([7, 3], [0.06, 0.02], 51) == 3
    assert g([7, 3], [0.05, 0.02], 51) == -1                             # 0.05 is strict
    assert g([7, 3], [0.06, 0.015], 51) == -1                            # 0.015 is strict
    assert g([7, 3], [np.nextafter(0.05, 1), np.nextafter(0.015, 1)], 51) == 3
    assert g([7, 3], [0.06, 0.02], 50) == -1                             # frame_index > 50 is strict
    assert g([7], [0.9], 80) == -1                                       # a second result is needed
    assert g([2, 9, 5], [0.06, 0.02, 0.02], 80) == 2                     # min_index starts from result 0
    assert g([9, 3, 5], [0.06, 0.01, 0.02], 80) == 5                     # a lower id counts only above 0.015
    assert g([9, 3, 5, 4], [0.06, 0.01, 0.012, 0.02], 80) == 4
    assert g([], [], 80) == -1


def test_ref_detect_queries_then_adds():
    voc = pr_cases.crafted()["k10L3"]
    db = pr_ref.Database(pr_ref.Tree(voc))
    d = pr_cases.descriptors_near(voc, 5, 100)
    loop, ids, scores = pr_ref.detect(db, d, 0)
    assert loop == -1 and len(ids) == 0 and len(scores) == 0 and db.size() == 1
    loop, ids, scores = pr_ref.detect(db, d, 60)                         # max_id 10: entry 0, and it is the last one as well
    assert ids.tolist() == [0] and abs(scores[0] - 1.0) < 1e-12 and loop == -1 and db.size() == 2


def test_ref_finds_the_revisits_of_mh05():
    """Calibration of the stream: detectLoop over the MH_05 world's keyframes with the k = 10, L = 5 test vocabulary."""
    m = pr_cases.mh05()
    assert uvs.api.check_vocabulary(m["voc"])[0] == abi.UVS_OK
    det = pr_cases.mh05_detections()
    p = m["world"]["p"]
    revisit = {k for k, _ in lc.mh05_candidates(m["world"])[0]}
    near = sum(1 for k, (loop, _, _) in enumerate(det) if loop >= 0 and k in revisit and np.linalg.norm(p[k] - p[loop]) < RADIUS)
    far = sum(1 for k, (loop, _, _) in enumerate(det) if loop >= 0 and np.linalg.norm(p[k] - p[loop]) >= RADIUS)
    print(f"MH_05: {near} revisiting keyframes with a candidate within {RADIUS} m, {far} of {len(det)} keyframes with one farther away")
    assert MH05_NEAR_RECORDED >= 20 and near >= 0.9 * MH05_NEAR_RECORDED
    assert far <= MH05_FAR_RECORDED + 1
    assert all(loop < k - 50 for k, (loop, _, _) in enumerate(det) if loop >= 0)


# ---------------------------------------------------------------- the device against pr_ref
def _check_transform(got, tree, desc):
    words, weights = pr_ref.transform(tree, desc)
    bw, bv = pr_ref.bow(words, weights)
    assert np.array_equal(got["words"], words) and bits_equal(got["weights"], weights)
    assert np.array_equal(got["bow_words"], bw) and bits_equal(got["bow_values"], bv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(pr_cases.crafted()))
def test_gpu_transform_on_the_crafted_trees(name):
    voc = pr_cases.crafted()[name]
    tree = pr_ref.Tree(voc)
    max_features = 4096 if name in ("k3L2", "stop") else 130
    pr = uvs.api.PlaceRecognizer(voc, max_features=max_features, initial_entries=4)
    frames = [pr_cases.descriptors_near(voc, 20 + i, n) for i, n in enumerate((0, 1, 63, 64, 65, max_features))]
    if name == "tie":
        frames[1] = pr_cases.TIE_QUERY
    got = pr.transform(frames)
    for g, d in zip(got, frames):
        _check_transform(g, tree, d)
    if name == "tie":
        assert got[1]["words"].tolist() == [pr_cases.TIE_WORD]
    assert pr.size() == 0
    rc, _ = pr.transform_raw([np.zeros((max_features + 1, 4), np.uint64)])
    assert rc == abi.UVS_ERR_CAPACITY
    pr.close()


@pytest.mark.gpu
def test_gpu_transform_500_descriptors_and_batches():
    voc = pr_cases.crafted()["k10L3"]
    tree = pr_ref.Tree(voc)
    pr = uvs.api.PlaceRecognizer(voc, max_features=600, initial_entries=4)
    d500 = np.r_[pr_cases.descriptors_near(voc, 30, 400), lc.random_desc(np.random.default_rng(31), 100)]
    _check_transform(pr.transform([d500])[0], tree, d500)
    frames = [pr_cases.descriptors_near(voc, 40 + i, n) for i, n in enumerate((17, 600, 0, 255, 321))]
    batch = pr.transform(frames)
    for g, d in zip(batch, frames):
        single = pr.transform([d])[0]
        for k in ("words", "bow_words"):
            assert np.array_equal(g[k], single[k]), k
        for k in ("weights", "bow_values"):
            assert bits_equal(g[k], single[k]), k
        _check_transform(g, tree, d)
    pr.close()


def _query_frames(voc):
    sizes = [120 + (37 * f) % 200 for f in range(70)]
    sizes[10] = 0
    return [pr_cases.descriptors_near(voc, 200 + f, n) for f, n in enumerate(sizes)]


@pytest.mark.gpu
def test_gpu_query_on_a_grown_database():
    voc = pr_cases.crafted()["k10L3"]
    frames = _query_frames(voc)
    db = pr_ref.Database(pr_ref.Tree(voc))
    pr = uvs.api.PlaceRecognizer(voc, max_features=400, initial_entries=8)      # the store doubles on the way to 70 entries
    assert len(pr.query([frames[0]], 4, -1)[0][0]) == 0 and len(pr.query([frames[0]], 0, -1)[0][0]) == 0      # an empty database answers nothing
    for f, d in enumerate(frames):
        assert pr.add([d])[0] == db.add(d) == f
    assert pr.size() == 70
    queries = [pr_cases.descriptors_near(voc, 300, 250), frames[33], np.zeros((0, 4), np.uint64), pr_cases.descriptors_near(voc, 301, 1)]
    for max_results in (1, 4, 0):
        for max_id in (-2, -1, 0, 69, 30, 10, 11, 200):
            got = pr.query(queries, max_results, max_id)
            for q, (ids, scores) in zip(queries, got):
                wi, ws = db.query(q, max_results, max_id)
                assert np.array_equal(ids, wi) and bits_equal(scores, ws), (max_results, max_id)
    got = pr.query(queries, 4, [-1, 5, -1, -2])                                  # a max_id per query
    for q, mid, (ids, scores) in zip(queries, (-1, 5, -1, -2), got):
        wi, ws = db.query(q, 4, mid)
        assert np.array_equal(ids, wi) and bits_equal(scores, ws)
    ids, scores = pr.query([frames[33]], 1, -1)[0]
    assert ids.tolist() == [33] and abs(scores[0] - 1.0) < 1e-12
    assert len(pr.query([queries[2]], 0, -1)[0][0]) == 0 and pr.size() == 70     # a zero-length query; queries change no state
    # the last entry is always eligible, and an entry without a common word is no result
    assert pr.query([frames[69]], 0, -2)[0][0].tolist() == [69]
    assert 10 not in pr.query([queries[0]], 0, -1)[0][0].tolist()
    pr.close()


@pytest.mark.gpu
def test_gpu_tie_goes_to_the_lower_entry():
    voc = pr_cases.crafted()["k10L3"]
    a, b = pr_cases.descriptors_near(voc, 400, 90), pr_cases.descriptors_near(voc, 401, 90)
    pr = uvs.api.PlaceRecognizer(voc, max_features=128, initial_entries=2)
    pr.add([b, a, b, a, b])
    db = pr_ref.Database(pr_ref.Tree(voc))
    for d in (b, a, b, a, b):
        db.add(d)
    for max_results in (0, 1, 2, 3):
        ids, scores = pr.query([a], max_results, -1)[0]
        wi, ws = db.query(a, max_results, -1)
        assert np.array_equal(ids, wi) and bits_equal(scores, ws)
    assert pr.query([a], 2, -1)[0][0].tolist() == [1, 3]
    pr.close()


@pytest.mark.gpu
def test_gpu_batch_add_equals_single_adds_and_clear_gives_a_fresh_handle():
    voc = pr_cases.crafted()["k10L3"]
    frames = _query_frames(voc)[:40]
    one = uvs.api.PlaceRecognizer(voc, max_features=400, initial_entries=8)
    many = uvs.api.PlaceRecognizer(voc, max_features=400, initial_entries=8)
    ids_one = [int(one.add([d])[0]) for d in frames]
    ids_many = many.add(frames[:3]).tolist() + many.add(frames[3:30]).tolist() + many.add(frames[30:]).tolist()
    assert ids_one == ids_many == list(range(40))
    queries = [pr_cases.descriptors_near(voc, 300, 250), frames[7]]
    want = one.query(queries, 0, -1)
    for got in (many.query(queries, 0, -1),):
        for (gi, gs), (wi, ws) in zip(got, want):
            assert np.array_equal(gi, wi) and bits_equal(gs, ws)
    # clear, then the second half only: a fresh handle's answers
    many.clear()
    assert many.size() == 0 and len(many.query(queries, 0, -1)[0][0]) == 0
    assert many.add(frames[20:]).tolist() == list(range(20))
    fresh = uvs.api.PlaceRecognizer(voc, max_features=400, initial_entries=8)
    fresh.add(frames[20:])
    for max_id in (-1, 5):
        for (gi, gs), (wi, ws) in zip(many.query(queries, 4, max_id), fresh.query(queries, 4, max_id)):
            assert np.array_equal(gi, wi) and bits_equal(gs, ws)
    for h in (one, many, fresh):
        h.close()


@pytest.mark.gpu
def test_gpu_detect_over_the_mh05_stream():
    m = pr_cases.mh05()
    want = pr_cases.mh05_detections()
    pr = uvs.api.PlaceRecognizer(m["voc"], max_features=4096, initial_entries=16)
    for k, d in enumerate(m["desc"]):
        loop, ids, scores = pr.detect(d, k)
        wl, wi, ws = want[k]
        assert loop == wl and np.array_equal(ids, wi) and bits_equal(scores, ws), k
    assert pr.size() == len(m["desc"]) and sum(w[0] >= 0 for w in want) > 100
    pr.close()


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.mark.gpu
def test_gpu_host_detect_loop_feeds_find_connection():
    """addKeyFrameDetectLoop (detectLoop on the GPU, then findConnection) accepts the loops addKeyFrameWithCandidate accepts when it is fed
    pr_ref's candidates."""
    m = pr_cases.mh05()
    W = m["world"]
    n = len(W["p"])
    cand = np.array([w[0] for w in pr_cases.mh05_detections()], np.int32)
    kf = W["kf"]
    nq = np.array([len(f["p3d"]) for f in kf], np.int32); nk = np.array([len(f["uv"]) for f in kf], np.int32)
    p3d = np.ascontiguousarray(np.concatenate([f["p3d"] for f in kf])); qd = np.ascontiguousarray(np.concatenate([f["qdesc"] for f in kf]))
    uv = np.ascontiguousarray(np.concatenate([f["uv"] for f in kf])); od = np.ascontiguousarray(np.concatenate([f["odesc"] for f in kf]))
    q = pg_ref.R_to_quat(W["Rv"]); tic, qic = np.ascontiguousarray(W["tic"]), np.ascontiguousarray(W["qic"])
    d = C.c_double; i32 = C.c_int32; u64 = C.c_uint64
    common = [0, n, _p(np.ascontiguousarray(W["stamps"]), d), _p(np.ascontiguousarray(W["pv"]), d), _p(q, d), _p(np.ones(n, np.int32), i32), _p(tic, d),
              _p(qic, d), _p(nq, i32), _p(p3d, d), _p(qd, u64), _p(nk, i32), _p(uv, d), _p(od, u64)]
    host = C.CDLL(HOST)
    host.uvs_host_pose_graph_detect_run.restype = C.c_int; host.uvs_host_pose_graph_verify_run.restype = C.c_int
    got_cand = np.zeros(n, np.int32)
    acc = np.zeros(n, np.int32); info = np.zeros((n, 8)); pose = np.zeros((n, 7))
    vargs, keep = abi.pr_vocabulary_args(m["voc"])
    rc = host.uvs_host_pose_graph_detect_run(*common, *vargs, _p(got_cand, i32), _p(acc, i32), _p(info, d), _p(pose, d))
    assert rc == abi.UVS_OK
    assert np.array_equal(got_cand, cand)
    acc2 = np.zeros(n, np.int32); info2 = np.zeros((n, 8)); pose2 = np.zeros((n, 7))
    rc = host.uvs_host_pose_graph_verify_run(*common, _p(cand, i32), _p(acc2, i32), _p(info2, d), _p(pose2, d))
    assert rc == abi.UVS_OK
    assert np.array_equal(acc, acc2) and acc.sum() >= 1
    assert np.array_equal(info, info2) and np.array_equal(pose, pose2)
