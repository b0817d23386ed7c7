"""The case table of tests/test_gpu_stream_order.py against include/s2s_hip.h: every exported function with a `void* stream` parameter
has a late-input case, the table names nothing else, every test it names exists, and every case that does not assert "returned
before the stream drained" cites words of the header that say the entry waits.  A new stream-taking entry fails here until it has a
case."""
import os
import re

import test_gpu_stream_order as G
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "s2s_hip.h")).read()


def stream_entries(header):
    """-> the names of the functions declared in the header (comments removed) that take a `void* stream`."""
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    out = []
    for m in re.finditer(r"\b(s2s_\w+)\s*\(([^;{}()]*)\)\s*;", code):
        params = " ".join(m.group(2).split())
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            out.append(m.group(1))
    return out


def test_the_parser_sees_what_a_reader_sees():
    names = stream_entries(HEADER)
    assert len(names) == len(set(names)) and len(names) >= 25
    assert {"s2s_predict_chunks", "s2s_kmer_model_events", "s2s_chunk_pack", "s2s_trainer_step"} <= set(names)
    assert not {"s2s_create", "s2s_stats_read", "s2s_kmer_model_events_host", "s2s_blow5_pack"} & set(names)
    assert HEADER.count("void* stream") == len(names)            # (no declaration escaped the pattern)
    assert stream_entries("int s2s_new_entry(int device,\n   void *stream, int n);\nint s2s_other(int n); /* void* stream */") == ["s2s_new_entry"]


def test_every_stream_taking_entry_has_a_case_and_nothing_else_is_named():
    names = stream_entries(HEADER)
    assert sorted(G.ENTRIES) == sorted(names), (sorted(set(names) - set(G.ENTRIES)), sorted(set(G.ENTRIES) - set(names)))
    for entry, tests in G.ENTRIES.items():
        assert tests, entry
        for t in tests:
            assert callable(getattr(G, t, None)) and t.startswith("test_"), (entry, t)


def test_every_case_that_may_wait_cites_the_header():
    flat = " ".join(re.sub(r"\n\s*\*", " ", HEADER).split())
    assert G.SYNCHRONISES
    for (entry, test), words in G.SYNCHRONISES.items():
        assert entry in G.ENTRIES and test in G.ENTRIES[entry], (entry, test)
        assert "synchronises" in words and " ".join(words.split()) in flat, (entry, words)
