"""validate + program_text over their whole input space against tests/golden/user_program_pins.json (recorded from the library before
csrc/user_problem.hip was split and its repetitions folded): every flag word gets the refusal it got, word for word, or the program
text it got, byte for byte; every launch layout and the clocked program likewise.  No GPU, nothing compiled."""
import json
import os

import pytest

from ddp_amd import _lib

import user_program_pins as pins

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "user_program_pins.json")


@pytest.fixture(scope="module")
def pinned():
    return pins.unpack(json.load(open(FIXTURE)))


@pytest.fixture(scope="module")
def now():
    return json.loads(json.dumps(pins.record(_lib.lib())))      # (through JSON: lists and string keys, as the fixture)


def test_the_sweeps_are_whole(pinned):
    """the fixture holds every flag word once per hook and shape, and every shape of the layout sweep"""
    assert len(pinned["flags"]) == 2 * len(pins.FLAG_SHAPES)
    for key, rec in pinned["flags"].items():
        words = sorted([w for ws in rec["refused"].values() for w in ws] + [int(w) for w in rec["accepted"]])
        assert words == sorted(pins.flag_words()), key
        assert rec["accepted"], key
    assert len(pinned["layout"]) == 2 * 32 * 8 + 2 * 4 * 6
    assert sum(isinstance(v, list) for v in pinned["layout"].values()) > 500
    assert all(isinstance(v, list) for v in pinned["clock"].values()) and len(pinned["clock"]) == 1


def test_every_flag_word_is_refused_or_accepted_as_before(pinned, now):
    assert sorted(now["flags"]) == sorted(pinned["flags"])
    for key, rec in pinned["flags"].items():
        got = now["flags"][key]
        assert sorted(got["refused"]) == sorted(rec["refused"]), key      # the messages, word for word
        for msg, words in rec["refused"].items():
            assert got["refused"][msg] == words, (key, msg)               # the FIRST message of every refused word
        assert sorted(got["accepted"]) == sorted(rec["accepted"]), key


def test_every_accepted_program_text_is_unchanged(pinned, now):
    for key, rec in pinned["flags"].items():
        for word, digest in rec["accepted"].items():
            assert now["flags"][key]["accepted"][word] == digest, (key, word)


def test_every_layout_and_the_clocked_program_are_unchanged(pinned, now):
    assert now["layout"] == pinned["layout"]
    assert now["clock"] == pinned["clock"]
