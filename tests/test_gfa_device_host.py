"""The parts of the device GFA parser that need no device: gfa.assemble_edges (events -> edges, torch sorts only) against read_gfa on the
goldens and on seeded adversarial files, and the argument rules of the new public names."""
import ctypes
import os

import pytest
import torch

from conftest import GOLDEN
from gfa_statement import adversarial_gfa, gfa_events
from gnnome_amd import gfa

GOLDEN_GFAS = ("g10_hifiasm8_utg.gfa", "g10_hifiasm7.gfa", "g10_raven6.gfa", "g14_single.gfa", "g14_multi.gfa", "g14_utg_x.gfa")


def _check_edges(path):
    want = gfa.read_gfa(path, similarity=None)
    u, v, ol, tag, num_nodes = gfa_events(path)
    assert num_nodes == want["num_nodes"]
    src, dst, overlap, tags = gfa.assemble_edges(u, v, ol, tag, num_nodes)
    assert torch.equal(src, want["src"]) and torch.equal(dst, want["dst"])
    assert torch.equal(overlap, want["overlap_length"])
    assert torch.equal(want["read_length"][src] - overlap, want["prefix_length"])
    if want["overlap_similarity"] is None:
        assert src.numel() == 0 or bool(torch.isnan(tags).any())
    else:
        assert torch.equal(tags.float(), want["overlap_similarity"])
    return src.numel()


@pytest.mark.parametrize("name", GOLDEN_GFAS)
def test_edge_assembly_on_the_goldens(name):
    assert _check_edges(os.path.join(GOLDEN, name)) > 0


@pytest.mark.parametrize("seed", range(20))
def test_edge_assembly_on_adversarial_files(tmp_path, seed):
    path = tmp_path / "adv.gfa"
    path.write_bytes(adversarial_gfa(seed, tags=("all", "all_but_one", "none")[seed % 3], sequences=bool(seed % 2)).encode("ascii"))
    assert _check_edges(str(path)) > 0


def test_edge_assembly_last_write_wins_first_position_stays():
    # (0,2) first at event 0, rewritten at events 3 and 4; (0,1) first at event 1: the order by first event puts (0,2) before (0,1)
    u = torch.tensor([0, 0, 3, 0, 0, 2])
    v = torch.tensor([2, 1, 1, 2, 2, 0])
    ol = torch.tensor([5, 6, 7, 8, 9, 4])
    src, dst, overlap, tag = gfa.assemble_edges(u, v, ol, torch.arange(6), 4)
    assert src.tolist() == [0, 0, 2, 3] and dst.tolist() == [2, 1, 0, 1]
    assert overlap.tolist() == [9, 6, 4, 7] and tag.tolist() == [4, 1, 5, 2]
    empty = torch.zeros(0, dtype=torch.int64)
    assert all(t.numel() == 0 for t in gfa.assemble_edges(empty, empty, empty, empty, 0))


def test_parser_argument_rules():
    path = os.path.join(GOLDEN, "g10_raven6.gfa")
    with pytest.raises(ValueError, match="parser"):
        gfa.read_gfa(path, similarity=None, parser="bogus")
    with pytest.raises(ValueError, match="read_gfa"):
        gfa.read_gfa_device(path, similarity=lambda a, b, n: 1.0)
    assert issubclass(gfa.GfaDeviceError, ValueError)
    a, b = gfa.read_gfa(path, similarity=None, keep_sequences=True), gfa.read_gfa(path, similarity=None, keep_sequences=True, parser="host")
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_pipeline_refuses_an_unknown_parser():
    from gnnome_amd import pipeline
    with pytest.raises(ValueError, match="parser"):
        pipeline.assemble(os.path.join(GOLDEN, "g10_raven6.gfa"), None, 10, device=torch.device("cpu"), scores=torch.zeros(1), parser="bogus")


def test_tile_constants_are_the_librarys():
    from gnnome_amd import _lib
    tok, pack = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.load().gnnome_gfa_tile_sizes(ctypes.byref(tok), ctypes.byref(pack)) == 0
    assert (tok.value, pack.value) == (gfa.TOKENISE_TILE, gfa.PACK_TILE)


def test_entries_validate_their_arguments_without_a_gpu():
    from gnnome_amd import _lib
    lib = _lib.load()
    assert lib.gnnome_gfa_mark(None, 10, None, None, None) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_gfa_classify(None, 10, None, None, 3, None, 2, None, None, None, None, None) == -1 and b"null" in lib.gnnome_last_error()
    one = (ctypes.c_int64 * 8)()
    ptr = ctypes.cast(one, ctypes.c_void_p)
    assert lib.gnnome_gfa_names_insert(ptr, 8, ptr, ptr, 4, ptr, 4, ptr, 1, ptr, None) == -1 and b"power of two" in lib.gnnome_last_error()
    assert lib.gnnome_gfa_names_insert(ptr, 8, ptr, ptr, 4, ptr, 6, ptr, 1, ptr, None) == -1 and b"power of two" in lib.gnnome_last_error()
    assert lib.gnnome_gfa_links(ptr, 8, ptr, ptr, 1, ptr, ptr, 4, ptr, 4, ptr, 1, ptr, ptr, ptr, None) == -1
    assert lib.gnnome_gfa_pack(None, 10, None, None, 2, None, 5, None) == -1 and b"null" in lib.gnnome_last_error()


def test_auto_answers_like_the_host_parser_with_or_without_a_device(tmp_path):
    path = os.path.join(GOLDEN, "g10_hifiasm8_utg.gfa")
    a, b = gfa.read_gfa(path, similarity=None, parser="auto"), gfa.read_gfa(path, similarity=None)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    bad = tmp_path / "bad.gfa"
    bad.write_text("S\ta\t*\tLN:i:5\nL\ta\t+\tnobody\t+\t3M\n")
    with pytest.raises(KeyError):
        gfa.read_gfa(str(bad), similarity=None, parser="auto")
