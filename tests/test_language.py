"""xworld_amd/language.py against the reference's CFG + task grammars (tests/golden/sentences.json).  CPU only."""
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASKS = {"XWorld3DNavTarget": 0, "XWorld3DNavTargetNear": 1, "XWorld3DNavTargetBetween": 2, "XWorld3DNavTargetDirection": 3,
         "XWorld3DNavTargetAvoid": 4, "XWorldNavTarget": 5, "XWorldNavColorTarget": 7}


@pytest.mark.parametrize("name", sorted(TASKS))
def test_sentences_match_reference_cfg(name):
    from xworld_amd import language
    with open(os.path.join(GOLD, "sentences.json")) as f:
        gold = json.load(f)
    kinds = set()
    for rec in gold["tasks"][name]:
        decisions = list(rec["decisions"])

        def choose(n, _d=decisions):
            v = _d.pop(0)
            assert 0 <= v < n
            return v
        got = language.GRAMMARS[TASKS[name]].expand(choose, dict(rec["bind"]))
        assert got == rec["sentence"], rec
        assert not decisions                                   # the same number of random.choice calls
        kinds.add(rec["bind"]["S"])
    assert "start" in kinds and len(kinds) >= 2


def test_philox_stream_matches_the_oracle(oracle):
    from xworld_amd import language
    for seed, gid, ep in ((0xC0FFEE, 0, 0), (1, 77, 3), (0xFFFFFFFF, 123456, 9)):
        import ctypes as C
        a = language.Stream(seed, gid, ep, 3)
        b = oracle.Stream()
        oracle.lib().orc_stream_init(C.byref(b), seed, gid, ep, 3)
        for n in (7, 5, 3, 4, 1, 2, 115, 6, 2):
            assert a.below(n) == oracle.lib().orc_stream_below(C.byref(b), n)


def test_library_sentences_equal_language_py():
    """xworld_amd/csrc/xwb_language.h (what xwb_sentence and the state packets use) against language.py, which the tests above pin
    to the reference's CFG: the same grammars, the same stream, the same draws -- sentence for sentence, no GPU needed."""
    import ctypes as C
    import random
    from xworld_amd import language, lib
    L = lib.load()
    names = ["apple", "avocado", "banana", "blueberry", "cabbage", "cauliflower", "cherry", "coconut", "cucumber", "fig"]
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])

    def c3(task, stage, event, a, b, direction, seed, gid, ep):
        need = C.c_size_t()
        lib.check(L.xwb_language_sentence(task, stage, event, arr, len(names), a, b, direction, seed, gid, ep, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        lib.check(L.xwb_language_sentence(task, stage, event, arr, len(names), a, b, direction, seed, gid, ep, buf, need.value, C.byref(need)))
        return buf.value.decode()

    def c2(task, timeup, name, color, seed, gid, ep, steps):
        need = C.c_size_t()
        lib.check(L.xwb_language_sentence_2d(task, timeup, name.encode(), color.encode(), seed, gid, ep, steps, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        lib.check(L.xwb_language_sentence_2d(task, timeup, name.encode(), color.encode(), seed, gid, ep, steps, buf, need.value, C.byref(need)))
        return buf.value.decode()

    rng = random.Random(7)
    seen = set()
    for i in range(3000):
        task = rng.randrange(5)
        seed, gid, ep = rng.getrandbits(32), rng.getrandbits(20), rng.randrange(500)
        a, b = rng.randrange(len(names)), rng.randrange(len(names))
        direction = rng.randrange(1, 5)
        want = language.sentence(task, 1, 0, names, a, b if task == 2 else 0xFFFF, direction if task == 3 else 0, seed, gid, ep)
        got = c3(task, 1, 0, a, b if task == 2 else 0xFFFF, direction if task == 3 else 0, seed, gid, ep)
        assert got == want != "", (task, seed, gid, ep)
        seen.add(got.split()[0])
    assert len(seen) >= 8                                  # the grammars' variety shows
    for task in range(5):
        for event in (1, 2, 3):
            assert c3(task, 2, event, 0xFFFF, 0xFFFF, 0, 1, 2, 3) == language.sentence(task, 2, event, names, 0xFFFF, 0xFFFF, 0, 1, 2, 3)
        assert c3(task, 2, 0, 0, 0xFFFF, 0, 1, 2, 3) == "" == c3(task, 1, 0, 0xFFFF, 0xFFFF, 0, 1, 2, 3)      # silent: terminal stage / nothing bound
    assert c3(6, 1, 0, 0, 0xFFFF, 0, 1, 2, 3) == ""        # a task without a grammar
    for i in range(1500):
        task = rng.choice((5, 7))
        seed, gid, ep, steps = rng.getrandbits(32), rng.getrandbits(20), rng.randrange(500), rng.randrange(60)
        name, color = rng.choice(names), rng.choice(["red", "green", "blue", "yellow"])
        assert c2(task, 0, name, color, seed, gid, ep, steps) == language.sentence_2d(task, name, color, seed, gid, ep, steps) != ""
    assert c2(5, 1, "", "", 0, 0, 0, 0) == language.sentence_2d_timeup(5) == "Time up ."


def _c_string(call):
    """a string hook's two-call protocol (size, then bytes) -> (rc, text)"""
    import ctypes as C
    need = C.c_size_t()
    rc = call(None, 0, C.byref(need))
    if rc:
        return rc, None
    buf = C.create_string_buffer(need.value)
    rc = call(buf, need.value, C.byref(need))
    return rc, buf.value.decode()


def test_2d_tasks_have_no_correct_or_wrong_message():
    """The 2-D-native grammars have no `correct` / `wrong` rule: asked for one through the 3-D hook, the teacher is silent."""
    import ctypes as C
    from xworld_amd import lib
    L = lib.load()
    arr = (C.c_char_p * 2)(b"apple", b"fig")
    for task in (5, 7):
        for stage in (0, 1, 2):
            for event in (1, 2):
                for a in (0, 0xFFFF):
                    rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence(task, stage, event, arr, 2, a, 0xFFFF, 0, 1, 2, 3,
                                                                                        out, cap, need))
                    assert rc == 0 and text == "", (task, stage, event, a)
        rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence(task, 0, 3, arr, 2, 0xFFFF, 0xFFFF, 0, 1, 2, 3, out, cap, need))
        assert rc == 0 and text == "Time up ."


def test_a_bound_name_with_white_space_is_an_argument_error():
    import ctypes as C
    from xworld_amd import lib
    L = lib.load()
    XWB_ERR_ARG = -1                                       # include/xwb.h
    for bad in (b"green apple", b"green\tapple", b"apple "):
        arr = (C.c_char_p * 2)(bad, b"fig")
        for task, a, b in ((0, 0, 0xFFFF), (1, 0, 0xFFFF), (2, 1, 0), (3, 0, 0xFFFF), (4, 0, 0xFFFF)):
            rc, _ = _c_string(lambda out, cap, need: L.xwb_language_sentence(task, 1, 0, arr, 2, a, b, 1, 1, 2, 3, out, cap, need))
            assert rc == XWB_ERR_ARG, (bad, task)
            assert "a name or colour is not one word" in L.xwb_last_error().decode()
        # the other name still makes a sentence, and the messages that bind no name are not affected
        rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence(0, 1, 0, arr, 2, 1, 0xFFFF, 0, 1, 2, 3, out, cap, need))
        assert rc == 0 and "fig" in text.split()
        rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence(0, 2, 1, arr, 2, 0, 0xFFFF, 0, 1, 2, 3, out, cap, need))
        assert rc == 0 and text == "Well done !"
        for task, name, color in ((5, bad, b"na"), (7, bad, b"red"), (7, b"fig", bad)):
            rc, _ = _c_string(lambda out, cap, need: L.xwb_language_sentence_2d(task, 0, name, color, 1, 2, 3, 4, out, cap, need))
            assert rc == XWB_ERR_ARG, (bad, task)
        rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence_2d(5, 1, bad, b"", 1, 2, 3, 4, out, cap, need))
        assert rc == 0 and text == "Time up ."


def test_strings_are_the_word_ids_looked_up():
    """xwb_language_sentence / _2d against xwb_language_sentence_ids under a vocabulary that holds every word, exact case: the
    ids mapped back through it are the string's words."""
    import ctypes as C
    import random
    from xworld_amd import language, lib
    L = lib.load()
    names = ["apple", "avocado", "banana", "blueberry", "cabbage", "cauliflower", "cherry", "coconut", "cucumber", "fig"]
    colors = ["red", "green", "blue", "yellow", "na"]
    words = set(names + colors)
    for g in language.GRAMMARS.values():
        for alts in g.rules.values():
            for alt in alts:
                words.update(s[1:-1] for s in alt if s.startswith("'"))
    vocab = ["<unk>"] + sorted(words)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    warr = (C.c_char_p * len(vocab))(*[w.encode() for w in vocab])
    rng = random.Random(99)
    spoke = 0
    for i in range(600):
        task = rng.choice((0, 1, 2, 3, 4, 5, 6, 7))
        two_d = task in (5, 7)
        stage, event = rng.choice(((1, 0), (1, 0), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3)))
        if two_d:
            stage, event = rng.choice(((1, 0), (1, 0), (0, 3)))
        seed, gid, ep, steps = rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), rng.randrange(1 << 16)
        a, b, direction = rng.randrange(len(names)), rng.randrange(len(names)), rng.randint(1, 4)
        color = rng.choice(colors).encode()
        if two_d:
            rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence_2d(task, int(event == 3), names[a].encode(), color, seed, gid,
                                                                                   ep, steps, out, cap, need))
        else:
            rc, text = _c_string(lambda out, cap, need: L.xwb_language_sentence(task, stage, event, arr, len(names), a, b, direction, seed,
                                                                                gid, ep, out, cap, need))
        assert rc == 0
        need = C.c_int32()
        buf = (C.c_int32 * 64)()
        lib.check(L.xwb_language_sentence_ids(task, stage, event, arr, len(names), a, b, direction, color, seed, gid, ep, steps, warr,
                                              len(vocab), 0, 0, buf, 64, C.byref(need)))
        ids = list(buf[:need.value])
        assert 0 not in ids
        assert " ".join(vocab[k] for k in ids) == text, (i, task, stage, event)
        spoke += bool(text)
    assert spoke >= 300
