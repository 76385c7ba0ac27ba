"""keto_list_encode_batch without a GPU: the entry points next to an unchanged ABI version, the error
paths that need no device, and the expectations of tests/list_encode_util.py pinned by hand-written
bytes (the GPU file compares the engine with them, and them with the host encoder keto_tree_json,
which needs an expand and so a device)."""
import ctypes as C
import os
import re

import pytest

import keto_amd
from keto_amd import capi
from tests import list_encode_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["keto_list_encode_batch", "keto_list_encoded_free", "keto_list_encoded_count",
                "keto_list_encoded_bytes", "keto_list_encoded_offsets", "keto_list_encoded_status",
                "keto_list_encoded_next_page", "keto_list_encoded_totals", "keto_list_encoded_tuples",
                "keto_list_encoded_timing"]
E_INVALID, E_HIP = -1, -2


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "keto_mi355x.h")).read()
    lib = keto_amd.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    assert re.search(r"typedef struct keto_list_encoded keto_list_encoded;", hdr)
    assert re.search(r"int keto_list_encode_batch\(keto_snapshot\* s, const keto_list_req\* reqs, uint32_t n,\s*"
                     r"uint32_t encoding[^,]*, keto_list_encoded\*\* out\);", hdr)
    # additive: the ABI version does not move, and the pinned name families gain nothing
    assert int(re.search(r"#define KETO_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.keto_abi_version() == 8 == capi.KETO_ABI_VERSION
    assert not any(n.startswith(("keto_subjects_", "keto_lookup_", "keto_looked_")) for n in ENTRY_POINTS)
    for name in ("list_encode_raw", "list_encode"):
        assert callable(getattr(keto_amd.Snapshot, name))


def _host_only():
    return keto_amd.Snapshot.build([(1, "n")], [(1, "a", "r", "u")], device=-1)


@pytest.mark.parametrize("queries", [[], [("n", "", "", None, 0, 0)]], ids=["n0", "n1"])
@pytest.mark.parametrize("encoding", U.ENCODINGS)
def test_host_only_snapshot_is_e_hip_whatever_n(queries, encoding):
    snap = _host_only()
    with pytest.raises(keto_amd.KetoError) as e:
        snap.list_encode(queries, encoding)
    assert e.value.code == E_HIP


def test_null_and_unknown_encoding_errors():
    snap = _host_only()
    lib = snap.lib
    keep = capi._Keep()
    reqs = snap._list_reqs(keep, [("n", "", "", None, 0, 0)])
    h = C.c_void_p()
    assert lib.keto_list_encode_batch(snap.h, reqs, C.c_uint32(1), C.c_uint32(capi.ENC_JSON), None) == E_INVALID
    assert lib.keto_list_encode_batch(snap.h, None, C.c_uint32(1), C.c_uint32(capi.ENC_JSON), C.byref(h)) == E_INVALID
    assert lib.keto_list_encode_batch(None, reqs, C.c_uint32(1), C.c_uint32(capi.ENC_JSON), C.byref(h)) == E_INVALID
    for enc in (2, 7, 0xFFFFFFFF):
        assert lib.keto_list_encode_batch(snap.h, reqs, C.c_uint32(1), C.c_uint32(enc), C.byref(h)) == E_INVALID
        assert lib.keto_list_encode_batch(snap.h, None, C.c_uint32(0), C.c_uint32(enc), C.byref(h)) == E_INVALID
    assert not h.value
    # reqs == NULL is fine with n == 0: the call gets as far as the missing device
    assert lib.keto_list_encode_batch(snap.h, None, C.c_uint32(0), C.c_uint32(capi.ENC_PROTO), C.byref(h)) == E_HIP
    # the accessors take NULL
    lib.keto_list_encoded_free(None)
    assert lib.keto_list_encoded_count(None) == 0
    total = C.c_uint64(5)
    assert not lib.keto_list_encoded_bytes(None, C.byref(total)) and total.value == 0
    for f in (lib.keto_list_encoded_offsets, lib.keto_list_encoded_status, lib.keto_list_encoded_next_page,
              lib.keto_list_encoded_totals, lib.keto_list_encoded_tuples):
        assert not f(None)
    assert lib.keto_list_encoded_timing(None, None, None, None) == E_INVALID


# ---------------------------------------------------------------------------------- go_json_string
# Hand-written from Go 1.17 encoding/json (encode.go, encodeState.string with escapeHTML): the short
# escapes, \u00XX for the other controls and < > &, DEL as it is, U+2028 / U+2029, one \ufffd per
# invalid byte, valid multi-byte sequences as they are.
HAND = {
    b'"': b'"\\""', b"\\": b'"\\\\"', b"\n": b'"\\n"', b"\r": b'"\\r"', b"\t": b'"\\t"',
    b"\x08": b'"\\u0008"', b"\x0c": b'"\\u000c"', b"\x00": b'"\\u0000"', b"\x01": b'"\\u0001"', b"\x1f": b'"\\u001f"',
    b" ": b'" "', b"\x7f": b'"\x7f"', b"<": b'"\\u003c"', b">": b'"\\u003e"', b"&": b'"\\u0026"', b"/": b'"/"', b"'": b'"\'"',
    b"\xe2\x80\xa8": b'"\\u2028"', b"\xe2\x80\xa9": b'"\\u2029"', b"\xe2\x80\xa7": b'"\xe2\x80\xa7"',
    b"\xe2\x80\xaa": b'"\xe2\x80\xaa"', b"\xc3\xa9": b'"\xc3\xa9"', b"\xe2\x82\xac": b'"\xe2\x82\xac"',
    b"\xf0\x9f\x98\x80": b'"\xf0\x9f\x98\x80"', b"\xf4\x8f\xbf\xbf": b'"\xf4\x8f\xbf\xbf"',
    b"\xc3": b'"\\ufffd"', b"\xc3(": b'"\\ufffd("', b"a\xc3": b'"a\\ufffd"', b"\xc0\x80": b'"\\ufffd\\ufffd"',
    b"\xe0\x80\x80": b'"\\ufffd\\ufffd\\ufffd"', b"\xf0\x80\x80\x80": b'"\\ufffd\\ufffd\\ufffd\\ufffd"',
    b"\xed\xa0\x80": b'"\\ufffd\\ufffd\\ufffd"', b"\xed\x9f\xbf": b'"\xed\x9f\xbf"',
    b"\xf4\x90\x80\x80": b'"\\ufffd\\ufffd\\ufffd\\ufffd"', b"\xf8\x88\x80\x80\x80": b'"' + b"\\ufffd" * 5 + b'"',
    b"\x80": b'"\\ufffd"', b"\xbf": b'"\\ufffd"', b"\xff": b'"\\ufffd"', b"\xe2\x82": b'"\\ufffd\\ufffd"',
    b"\xf0\x9f\x98": b'"\\ufffd\\ufffd\\ufffd"', b"": b'""', b"plain": b'"plain"',
    b'a"b\\c\nd<e>f&g\xc3h\xe2\x80\xa8i': b'"a\\"b\\\\c\\nd\\u003ce\\u003ef\\u0026g\\ufffdh\\u2028i"',
}


def test_go_json_string_escape_table():
    assert set(U.ESCAPE_CASES) == set(HAND)                  # every case of the table is pinned here
    for s in U.ESCAPE_CASES:
        assert U.go_json_string(s) == HAND[s], s


def test_rename_is_one_to_one_and_holds_every_escape_class():
    vals = list(U.RENAME.values())
    assert len(set(vals)) == len(vals) and not set(vals) & {k.encode() for k in U.RENAME}
    blob = b"\x00".join(vals)
    for piece in (b'"', b"\\", b"\n", b"\t", b"\x01", b"\x7f", b"<", b">", b"&", "\u2028".encode(), "é".encode(),
                  "€".encode(), "\U0001F600".encode(), b"\xc3", b"\xc0\x80", b"\xed\xa0\x80"):
        assert piece in blob, piece
    assert b"" in vals
    # the store's text keeps the order of the bytes
    texts = sorted(U.sql_text(v).encode("utf-8") for v in vals)
    assert [U.raw_bytes(t.decode("utf-8")) for t in texts] == sorted(vals)


# ---------------------------------------------------------------------------------- hand-worked bodies
TWO = [("n", "o", "r", ("id", "u")), ("n", "o", "r", ("set", "m", "p", "s"))]


def test_hand_worked_json():
    assert U.response_json(TWO, "2") == (
        b'{"relation_tuples":['
        b'{"namespace":"n","object":"o","relation":"r","subject_id":"u"},'
        b'{"namespace":"n","object":"o","relation":"r","subject_set":{"namespace":"m","object":"p","relation":"s"}}'
        b'],"next_page_token":"2"}')
    assert U.response_json([], "") == b'{"relation_tuples":[],"next_page_token":""}'
    assert U.response_json([("", "", "", ("id", ""))], "") == (
        b'{"relation_tuples":[{"namespace":"","object":"","relation":"","subject_id":""}],"next_page_token":""}')


def test_hand_worked_proto():
    want = bytes([
        0x0A, 0x0E,                          # relation_tuples[0]: 14 bytes
        0x0A, 0x01, ord("n"), 0x12, 0x01, ord("o"), 0x1A, 0x01, ord("r"),
        0x22, 0x03, 0x0A, 0x01, ord("u"),    # subject { id: "u" }
        0x0A, 0x16,                          # relation_tuples[1]: 22 bytes
        0x0A, 0x01, ord("n"), 0x12, 0x01, ord("o"), 0x1A, 0x01, ord("r"),
        0x22, 0x0B, 0x12, 0x09,              # subject { set { ... } }: 11 and 9 bytes
        0x0A, 0x01, ord("m"), 0x12, 0x01, ord("p"), 0x1A, 0x01, ord("s"),
        0x12, 0x01, ord("2"),                # next_page_token: "2"
    ])
    assert U.response_proto(TWO, "2") == want
    assert U.response_proto([], "") == b""
    # empty strings are left out, the id of the oneof is not; an empty set keeps its two headers
    assert U.response_proto([("", "", "", ("id", ""))], "") == bytes([0x0A, 0x04, 0x22, 0x02, 0x0A, 0x00])
    assert U.response_proto([("", "o", "", ("set", "", "", ""))], "10") == bytes(
        [0x0A, 0x07, 0x12, 0x01, ord("o"), 0x22, 0x02, 0x12, 0x00, 0x12, 0x02, ord("1"), ord("0")])


def test_response_proto_round_trips_through_the_parser():
    tuples = TWO + [(b"", U.RENAME["u"], b"r", ("id", U.RENAME["w"])), ("n", "x" * 200, "r", ("set", "", "y" * 17000, ""))]
    for token in ("", "9", "10", "100"):
        raw = U.response_proto(tuples, token)
        m = U.ListResponseMsg.FromString(raw)
        assert m.next_page_token == token.encode() and len(m.relation_tuples) == len(tuples)
        for got, t in zip(m.relation_tuples, tuples):
            assert (got.namespace, got.object, got.relation) == tuple(U._b(x) for x in t[:3])
            assert got.subject.WhichOneof("ref") == t[3][0]
            if t[3][0] == "id":
                assert got.subject.id == U._b(t[3][1])
            else:
                s = got.subject.set
                assert (s.namespace, s.object, s.relation) == tuple(U._b(x) for x in t[3][1:])
        assert m.SerializeToString(deterministic=True) == raw and m.ByteSize() == len(raw)
