"""The inverse-telecine rule's own property (tests/ivtc_ref.py), in numpy alone: film frames with
horizontal motion and per-sample noise below T go through 2:3 pulldown in every format, both field orders and all five phases,
and the reference gives them back byte for byte, in order, 16 for 20, with no repeat.

What the rule does not promise, and this test writes down: a stream that starts inside a pulldown cycle can start with an
ORPHAN frame, one whose partner field is not in the stream (phases 1 and 2).  Whatever it is matched with, it stays combed, is reported combed and, with
the policy `keep`, is delivered as woven.  At phase 1 the first cycle of five then holds five different frames and still loses one:
a film frame is lost there, once, at the start of the stream."""
import numpy as np
import pytest

import ivtc_ref as ref

H, W, N = 16, 48, 20


def film_index(frame, film):
    hits = [i for i, f in enumerate(film) if np.array_equal(frame, f)]
    return hits[0] if hits else -1


@pytest.mark.parametrize("fmt", ref.FORMATS)
@pytest.mark.parametrize("order", ["tff", "bff"])
def test_pulldown_gives_the_film_frames_back(fmt, order):
    film = ref.film_frames(fmt, 24, H, W, seed=3)
    assert len({f.tobytes() for f in film}) == 24
    for phase in range(5):
        video, src = ref.pulldown(film, fmt, H, W, N, phase, order)
        out, info = ref.detelecine(video, fmt, H, W, order, combed="keep")
        assert len(out) == 16 and info["stats"][:2] == (20, 16) and info["stats"][6] == 4, (fmt, order, phase)
        ids = [film_index(f, film) for f in out]
        orphans = [k for k, i in enumerate(ids) if i < 0]
        # at most two orphans, at the very start, each a frame of mixed fields whose partner is not in the stream, reported combed
        assert len(orphans) <= 2 and orphans == list(range(len(orphans))), (fmt, order, phase, ids)
        for k in orphans:
            assert src[k][0] != src[k][1] and info["combed"][k]
        assert not any(info["combed"][len(orphans):]), (fmt, order, phase)
        # film frames byte for byte, in order, no repeat
        rest = ids[len(orphans):]
        assert all(b > a for a, b in zip(rest, rest[1:])), (fmt, order, phase, ids)
        # and none is missing, except one in the first cycle of a stream that starts with an orphan
        missing = set(range(rest[0], rest[-1] + 1)) - set(rest)
        assert len(missing) <= (1 if orphans else 0) and all(m < rest[0] + 5 for m in missing), (fmt, order, phase, ids)
        if phase in (0, 3, 4):
            assert not orphans and not missing
        # the progressive frames of the stream pass through as matches of c
        assert all(m == "c" for m, (a, b) in zip(info["match"], src) if a == b)


def test_a_still_scene_passes_through():
    fmt = "yuv420p"
    f = ref.film_frames(fmt, 1, H, W)[0]
    out, info = ref.detelecine([f] * 7, fmt, H, W)
    assert info["match"] == "c" * 7 and not any(info["combed"]) and info["kept"] == [0, 2, 3, 4, 5, 6]
    assert all(np.array_equal(o, f) for o in out)


def test_decimation():
    big = ref.FIRST_DIFF
    assert ref.decimate([big, 5, 3, 3, 9]) == [0, 1, 3, 4]                  # ties drop the earliest
    assert ref.decimate([big, 5, 3, 4]) == [0, 1, 2, 3]                     # a trailing cycle loses none
    assert ref.decimate([big, 1, 1, 1, 1, 0, 9, 9, 9, 9, 7]) == [0, 2, 3, 4, 6, 7, 8, 9, 10]
    assert ref.decimate([big, 0, 0, 0, 0, 0], keep_all=True) == list(range(6))
    for n in range(23):
        assert len(ref.decimate([big] + [1] * (n - 1) if n else [])) == n - n // 5
