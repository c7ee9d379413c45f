"""textscan's host side: the rule for which decline a file is reported with, on plain ints, and the three readers' error classes
against the messages they have always had."""
import pytest

from gnnome_amd import gfa, maf, reads, textscan


def test_byte_level_finding_comes_before_the_lines_code_on_one_line():
    assert textscan.choose_decline([(4, 12)], (4, 3)) == (4, 12)
    assert textscan.choose_decline([(4, 13), (4, 12)], (4, 3)) == (4, 12)     # two byte-level findings on one line: the smaller code
    assert textscan.choose_decline([], (4, 3), extra=[(4, 2, 8)]) == (4, 3)   # and the line's code before a reader's extra candidate


def test_the_smaller_line_wins_whatever_its_rank():
    assert textscan.choose_decline([(7, 12)], (2, 5)) == (2, 5)
    assert textscan.choose_decline([(1, 13)], (2, 5)) == (1, 13)
    assert textscan.choose_decline([(7, 12)], (5, 3), extra=[(0, 2, 8)]) == (0, 8)
    assert textscan.choose_decline([(7, 12), (3, 13)], None) == (3, 13)


def test_no_finding_is_none():
    assert textscan.choose_decline([], None) is None
    assert textscan.choose_decline([], None, extra=[]) is None


def test_extra_candidates_are_honoured():
    assert textscan.choose_decline([], None, extra=[(9, 2, 8)]) == (9, 8)
    assert textscan.choose_decline([], (9, 4), extra=[(3, 2, 8), (6, 2, 8)]) == (3, 8)
    assert textscan.choose_decline([(0, 12)], None, extra=[(0, 2, 8)]) == (0, 12)


READER = " - not served by the device reader (parser='host' or 'auto')"
MESSAGES = [
    (reads.ReadsDeviceError, ("r.fq", 7, "a byte >= 0x80"), "r.fq: line 7: a byte >= 0x80" + READER),
    (reads.ReadsDeviceError, ("r.fq", 0, "the name table is full"), "r.fq: the name table is full" + READER),
    (maf.MafDeviceError, ("s.maf", 12, "a strand other than + or -"), "s.maf: line 12: a strand other than + or -" + READER),
    (maf.MafDeviceError, ("s.maf", 0, "a file above max_bytes (10 > 5)"), "s.maf: a file above max_bytes (10 > 5)" + READER),
    (gfa.GfaDeviceError, ("a.gfa", 3, "an L line without 6, 7 or 8 fields"),
     "a.gfa: line 3: an L line without 6, 7 or 8 fields - not served by the device parser (read_gfa(parser='host') or 'auto')"),
]


@pytest.mark.parametrize("cls,args,text", MESSAGES, ids=[f"{m[0].__name__}-line{m[1][1]}" for m in MESSAGES])
def test_error_classes_keep_their_messages(cls, args, text):
    e = cls(*args)
    assert str(e) == text and e.args == (text,)
    assert e.line == args[1] and e.reason == args[2]
    assert issubclass(cls, ValueError) and isinstance(e, textscan.DeviceDecline)
    assert cls is not textscan.DeviceDecline and len({reads.ReadsDeviceError, maf.MafDeviceError, gfa.GfaDeviceError}) == 3
