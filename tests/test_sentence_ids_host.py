"""xwb_language_sentence_ids -- the host run of the walk behind BatchedSimulator.sentence_ids (the same grammar tables,
the same expansion code as the device kernel) -- against xworld_amd/language.py tokenised through a vocabulary.  language.py is pinned to the
reference's CFG by tests/golden/sentences.json (test_language.py).  CPU only.

The vocabularies are the reference's dict files (tests/golden/nav_2d.txt, nav_3d.txt: byte-for-byte copies; they lack the shape
names and the colour words, which must come out as unk) and one built from the grammars' own words (no unk at all)."""
import ctypes as C
import os
import random

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASKS_3D = (0, 1, 2, 3, 4)
TASKS_2D = (5, 7)
XWB_ERR_ARG = -1                                      # include/xwb.h


def _L():
    from xworld_amd import lib
    return lib.load()


def _names():
    from xworld_amd import assets
    pal = assets.Palette(assets.MAP_CLASSES["XWorldWalls"]["subtrees"])       # animals, fruit and the shapes
    colors = sorted({m.get("color", "na") for m in pal.meta})
    return pal.names["goal"], colors


def _fold(w, fold):
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in w) if fold else w


def _grammar_words(fold):
    from xworld_amd import language
    words = set()
    for g in language.GRAMMARS.values():
        for alts in g.rules.values():
            for alt in alts:
                words.update(_fold(s[1:-1], fold) for s in alt if s.startswith("'"))
    names, colors = _names()
    words.update(_fold(w, fold) for w in names + colors)
    return ["<unk>"] + sorted(words)


def _vocabs():
    from xworld_amd.batched import read_vocabulary
    out = []
    for fold in (True, False):
        out.append(("nav_2d", read_vocabulary(os.path.join(GOLD, "nav_2d.txt")), 0, fold))
        out.append(("nav_3d", read_vocabulary(os.path.join(GOLD, "nav_3d.txt")), 0, fold))
        out.append(("grammar", _grammar_words(fold), 0, fold))
    return out


class Twin:
    def __init__(self, words, unk, fold):
        from xworld_amd import lib
        self.L, self.lib = _L(), lib
        self.words, self.unk, self.fold = list(words), unk, fold
        self.ids = {}
        for i, w in enumerate(self.words):
            if w:
                self.ids[_fold(w, fold)] = i
        self.names, self.colors = _names()
        self._w = (C.c_char_p * len(self.words))(*[w.encode() for w in self.words])
        self._n = (C.c_char_p * len(self.names))(*[n.encode() for n in self.names])

    def tokenise(self, sentence):
        return [self.ids.get(_fold(w, self.fold), self.unk) for w in sentence.split()]

    def call(self, task, stage=1, event=0, a=0, b=0, direction=0, color=None, seed=1, gid=0, ep=0, steps=0, cap=64):
        need = C.c_int32()
        buf = (C.c_int32 * max(cap, 1))()
        col = color.encode() if color is not None else None
        rc = self.L.xwb_language_sentence_ids(task, stage, event, self._n, len(self.names), a, b, direction, col, seed, gid, ep, steps,
                                              self._w, len(self.words), self.unk, 1 if self.fold else 0, buf, cap, C.byref(need))
        self.lib.check(rc)
        return list(buf[:min(need.value, cap)]), need.value


def _expect_3d(tw, task, stage, event, a, b, direction, seed, gid, ep):
    from xworld_amd import language
    return tw.tokenise(language.sentence(task, stage, event, tw.names, a, b, direction, seed, gid, ep))


def _expect_2d(tw, task, timeup, a, color, seed, gid, ep, steps):
    from xworld_amd import language
    s = language.sentence_2d_timeup(task) if timeup else language.sentence_2d(task, tw.names[a], color, seed, gid, ep, steps)
    return tw.tokenise(s)


@pytest.mark.parametrize("vocab", _vocabs(), ids=lambda v: "%s-%s" % (v[0], "fold" if v[3] else "exact"))
def test_every_stage_event_direction_and_name_slot(vocab):
    _, words, unk, fold = vocab
    tw = Twin(words, unk, fold)
    n = len(tw.names)
    seen = 0
    for task in TASKS_3D + (6, 8):
        for stage in (0, 1, 2):
            for event in (0, 1, 2, 3):
                for direction in ((1, 2, 3, 4) if task == 3 else (0,)):
                    for a, b in ((0, 1), (n - 1, 0), (7, n - 2)):          # both name slots, first and last names
                        for ep in (0, 5):
                            want = _expect_3d(tw, task, stage, event, a, b, direction, 0xC0FFEE, 11 + a, ep)
                            got, need = tw.call(task, stage, event, a, b, direction, None, 0xC0FFEE, 11 + a, ep)
                            assert got == want and need == len(want), (task, stage, event, direction, a, b, ep)
                            seen += bool(want)
    assert seen > 0
    for task in TASKS_2D:
        for timeup in (False, True):
            for a in (0, n - 1):
                for color in tw.colors:
                    for steps in (0, 1, 9):
                        want = _expect_2d(tw, task, timeup, a, color, 7, 3 + a, 2, steps)
                        got, need = tw.call(task, 0, 3 if timeup else 0, a, 0, 0, color, 7, 3 + a, 2, steps)
                        assert got == want and need == len(want), (task, timeup, a, color, steps)


def test_random_tuples_against_language_py():
    rng = random.Random(1234)
    vocabs = _vocabs()
    twins = [Twin(w, u, f) for _, w, u, f in vocabs]
    checked = 0
    for i in range(2400):
        tw = twins[i % len(twins)]
        n = len(tw.names)
        task = rng.choice(TASKS_3D + TASKS_2D)
        seed, gid, ep, steps = rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.randrange(0, 1 << 20)
        if task in TASKS_2D:
            a, color = rng.randrange(n), rng.choice(tw.colors)
            want = _expect_2d(tw, task, False, a, color, seed, gid, ep, steps)
            got, need = tw.call(task, 1, 0, a, 0, 0, color, seed, gid, ep, steps)
        else:
            a, b = rng.randrange(n), rng.randrange(n)
            direction = rng.randint(1, 4) if task == 3 else 0
            want = _expect_3d(tw, task, 1, 0, a, b, direction, seed, gid, ep)
            got, need = tw.call(task, 1, 0, a, b, direction, None, seed, gid, ep)
        assert got == want and need == len(want), (i, task, seed, gid, ep, steps)
        checked += 1
    assert checked >= 2000


def test_grammar_vocabulary_has_no_unk():
    for fold in (True, False):
        tw = Twin(_grammar_words(fold), 0, fold)
        rng = random.Random(5)
        for i in range(300):
            task = rng.choice(TASKS_3D + TASKS_2D)
            a, b = rng.randrange(len(tw.names)), rng.randrange(len(tw.names))
            got, need = tw.call(task, 1, 0, a, b, rng.randint(1, 4), rng.choice(tw.colors), rng.getrandbits(32), i, i % 7, i)
            assert need > 0 and 0 not in got, (task, got)


def test_words_outside_the_vocabulary_are_unk():
    """nav_2d.txt has neither the colour words nor the shape names the walls palette uses: they come out as unk."""
    from xworld_amd.batched import read_vocabulary
    words = read_vocabulary(os.path.join(GOLD, "nav_2d.txt"))
    unk = words.index("$")
    tw = Twin(words, unk, True)
    assert "red" not in words and "circle" not in words
    shapes = [tw.names.index(s) for s in ("circle", "square", "star", "triangle")]
    for s in shapes:
        for task, color in ((7, "red"), (5, "na")):
            got, _ = tw.call(task, 1, 0, s, 0, 0, color, 3, s, 1, 4)
            assert got.count(unk) == (2 if task == 7 else 1), (task, got)        # ColorTarget: colour and shape; Target: shape
            assert got == _expect_2d(tw, task, False, s, color, 3, s, 1, 4)
    # a known word is not unk: "apple" is in the dict
    a = tw.names.index("apple")
    got, _ = tw.call(0, 1, 0, a, 0, 0, None, 3, 1, 1)
    assert words.index("apple") in got and unk not in got


def test_truncation_reports_the_full_length():
    tw = Twin(_grammar_words(True), 0, True)
    full, need = tw.call(3, 1, 0, 2, 0, 3, None, 9, 9, 9)
    assert need == len(full) > 3
    got, need2 = tw.call(3, 1, 0, 2, 0, 3, None, 9, 9, 9, cap=3)
    assert got == full[:3] and need2 == need


def test_argument_errors():
    L = _L()
    names = (C.c_char_p * 2)(b"apple", b"fig")
    need = C.c_int32()
    buf = (C.c_int32 * 8)()

    def call(words, n, unk, fold=1, goal=names, n_goal=2):
        return L.xwb_language_sentence_ids(0, 1, 0, goal, n_goal, 0, 1, 0, None, 1, 2, 3, 0, words, n, unk, fold, buf, 8, C.byref(need))

    ok = (C.c_char_p * 3)(b"apple", b"go", b"to")
    assert call(ok, 3, 0) == 0
    assert call((C.c_char_p * 3)(b"go", b"to", b"go"), 3, 0) == XWB_ERR_ARG                  # duplicate
    assert call((C.c_char_p * 3)(b"Go", b"to", b"go"), 3, 0, fold=1) == XWB_ERR_ARG          # duplicate after folding
    assert call((C.c_char_p * 3)(b"Go", b"to", b"go"), 3, 0, fold=0) == 0
    assert call((C.c_char_p * 3)(b"go", None, b"to"), 3, 0) == XWB_ERR_ARG                   # NULL word
    assert call(ok, 0, 0) == XWB_ERR_ARG                                                     # n_words <= 0
    assert call(ok, -2, 0) == XWB_ERR_ARG
    assert call(ok, 3, 3) == XWB_ERR_ARG                                                     # unk outside the vocabulary
    assert call(ok, 3, -1) == XWB_ERR_ARG
    assert call(None, 3, 0) == XWB_ERR_ARG
    # a bound name is one vocabulary entry: names with whitespace (or empty ones) cannot be looked up as one word
    assert call(ok, 3, 0, goal=(C.c_char_p * 2)(b"green apple", b"fig")) == XWB_ERR_ARG
    assert call(ok, 3, 0, goal=(C.c_char_p * 2)(b"", b"fig")) == XWB_ERR_ARG
    assert call(ok, 3, 0, goal=(C.c_char_p * 2)(None, b"fig")) == XWB_ERR_ARG


def test_dict_file_loader_numbers_lines(tmp_path):
    from xworld_amd import language
    from xworld_amd.batched import read_vocabulary
    p = tmp_path / "d.txt"
    p.write_text("$\n-\n  go \n\nto\nWell\n")
    assert read_vocabulary(str(p)) == ["$", "-", "go", "", "to", "Well"]
    words = read_vocabulary(os.path.join(GOLD, "nav_2d.txt"))
    with open(os.path.join(GOLD, "nav_2d.txt")) as f:
        lines = f.read().split("\n")
    assert len(words) == 165 and words[:2] == ["$", "-"]
    for i, w in enumerate(words):
        assert lines[i].strip() == w
    # blank entries keep their ids and match nothing: the twin numbers words exactly as the loader does
    tw = Twin(["", "<unk>", "", "go", "to", "apple"], 1, True)
    got, _ = tw.call(0, 1, 0, 0, 0, 0, None, 1, 1, 0)
    assert set(got) <= {1, 3, 4, 5}
    assert got == tw.tokenise(language.sentence(0, 1, 0, tw.names, 0, 0, 0, 1, 1, 0))
