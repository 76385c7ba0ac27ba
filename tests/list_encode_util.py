"""What keto_list_encode_batch must produce, restated from the reference (paths relative to its tree)
without any code under test: expectations only.

  * JSON       json.Marshal(GetResponse) (internal/relationtuple/handler.go:23-29); a tuple marshals as
               its RelationQuery (definitions.go:340-342,367-375 and :45-65: namespace, object, relation,
               then subject_id or subject_set, omitempty on those two only); an empty page is []
               (internal/persistence/sql/relationtuples.go:267).  Strings as Go 1.17 encoding/json writes
               them with HTML escaping on (encode.go, encodeState.string).
  * protobuf   proto.Marshal(ListRelationTuplesResponse) (read_server.go:39-45,148-151; ToProto,
               definitions.go:231-250,358-365) through message classes built at run time from a
               descriptor that restates acl.proto:14-52 and read_service.proto:85-91, as
               tests/proto_util.py does for SubjectTree.  The restated fields are `bytes` where the
               .proto says `string`: the wire format is the same (length-delimited, left out when
               empty, a oneof member present even when empty) and the Python runtime then takes the
               names of RENAME that are not valid UTF-8, which the engine copies as they are.

Strings are bytes throughout.  The SQLite oracle store only holds text, so a byte string goes into
it as its Latin-1 decoding (sql_text) and comes back through raw_bytes: SQLite's BINARY collation
compares the UTF-8 of that text, and Latin-1 -> UTF-8 keeps the order of the original bytes (a byte
below 0x80 stays, 0x80..0xBF become C2 xx, 0xC0..0xFF become C3 xx: monotone, and prefixes stay
prefixes), so both sides order the same strings the same way."""
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

from oracle.oracle_sql import RelationTuple, SQLStore, SubjectID, SubjectSet
from tests import list_util
from tests.randgraph import random_graph

ENC_PROTO, ENC_JSON = 0, 1
ENCODINGS = ("json", "proto")

_HEX = "0123456789abcdef"


def _decode_rune(s: bytes, i: int):
    """utf8.DecodeRune at s[i:]: (code point, width), (0xFFFD, 1) for an invalid sequence."""
    c = s[i]
    n = 2 if c >> 5 == 6 else 3 if c >> 4 == 14 else 4 if c >> 3 == 30 else 0
    if n == 0 or i + n > len(s):
        return 0xFFFD, 1
    cp = c & (0x7F >> n)
    for k in range(1, n):
        if s[i + k] >> 6 != 2:
            return 0xFFFD, 1
        cp = (cp << 6) | (s[i + k] & 0x3F)
    if cp < (0x80, 0x800, 0x10000)[n - 2] or cp > 0x10FFFF or 0xD800 <= cp <= 0xDFFF:
        return 0xFFFD, 1
    return cp, n


def go_json_string(s: bytes) -> bytes:
    """encodeState.string(s, escapeHTML=true) of Go 1.17: the quoted JSON text of a Go string."""
    out = bytearray(b'"')
    i = 0
    while i < len(s):
        b = s[i]
        if b < 0x80:
            if b in b'"\\':
                out += b"\\" + bytes([b])
            elif b == 0x0A:
                out += b"\\n"
            elif b == 0x0D:
                out += b"\\r"
            elif b == 0x09:
                out += b"\\t"
            elif b < 0x20 or b in b"<>&":
                out += b"\\u00" + bytes([ord(_HEX[b >> 4]), ord(_HEX[b & 15])])     # \b and \f too
            else:
                out.append(b)
            i += 1
            continue
        cp, w = _decode_rune(s, i)
        if cp == 0xFFFD and w == 1:
            out += b"\\ufffd"
        elif cp in (0x2028, 0x2029):
            out += b"\\u202" + bytes([ord(_HEX[cp & 15])])
        else:
            out += s[i:i + w]
        i += w
    out += b'"'
    return bytes(out)


def _b(x) -> bytes:
    return x if isinstance(x, bytes) else x.encode()


def tuple_json(t) -> bytes:
    """t = (namespace, object, relation, ("id", id) | ("set", namespace, object, relation))."""
    ns, obj, rel, sub = t
    out = (b'{"namespace":' + go_json_string(_b(ns)) + b',"object":' + go_json_string(_b(obj)) + b',"relation":' +
           go_json_string(_b(rel)))
    if sub[0] == "id":
        return out + b',"subject_id":' + go_json_string(_b(sub[1])) + b"}"
    return (out + b',"subject_set":{"namespace":' + go_json_string(_b(sub[1])) + b',"object":' +
            go_json_string(_b(sub[2])) + b',"relation":' + go_json_string(_b(sub[3])) + b"}}")


def response_json(tuples, token="") -> bytes:
    return (b'{"relation_tuples":[' + b",".join(tuple_json(t) for t in tuples) + b'],"next_page_token":"' +
            _b(token) + b'"}')


def _classes():
    F = descriptor_pb2.FieldDescriptorProto
    pkg = "ory.keto.acl.v1alpha1"
    fd = descriptor_pb2.FileDescriptorProto(name="keto_list_restated.proto", package=pkg, syntax="proto3")
    ss = fd.message_type.add(name="SubjectSet")
    for i, n in enumerate(("namespace", "object", "relation"), 1):
        ss.field.add(name=n, number=i, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    sub = fd.message_type.add(name="Subject")
    sub.oneof_decl.add(name="ref")
    sub.field.add(name="id", number=1, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL, oneof_index=0)
    sub.field.add(name="set", number=2, type=F.TYPE_MESSAGE, label=F.LABEL_OPTIONAL, oneof_index=0,
                  type_name=f".{pkg}.SubjectSet")
    rt = fd.message_type.add(name="RelationTuple")
    for i, n in enumerate(("namespace", "object", "relation"), 1):
        rt.field.add(name=n, number=i, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    rt.field.add(name="subject", number=4, type=F.TYPE_MESSAGE, label=F.LABEL_OPTIONAL, type_name=f".{pkg}.Subject")
    lr = fd.message_type.add(name="ListRelationTuplesResponse")
    lr.field.add(name="relation_tuples", number=1, type=F.TYPE_MESSAGE, label=F.LABEL_REPEATED,
                 type_name=f".{pkg}.RelationTuple")
    lr.field.add(name="next_page_token", number=2, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    get = getattr(message_factory, "GetMessageClass", None)
    if get is None:
        f = message_factory.MessageFactory(pool)
        get = lambda d: f.GetPrototype(d)
    return (get(pool.FindMessageTypeByName(f"{pkg}.RelationTuple")),
            get(pool.FindMessageTypeByName(f"{pkg}.ListRelationTuplesResponse")))


RelationTupleMsg, ListResponseMsg = _classes()


def fill_tuple(m, t):
    ns, obj, rel, sub = t
    m.namespace, m.object, m.relation = _b(ns), _b(obj), _b(rel)
    if sub[0] == "id":
        m.subject.id = _b(sub[1])                          # ToProto always sets the oneof
    else:
        m.subject.set.SetInParent()
        m.subject.set.namespace, m.subject.set.object, m.subject.set.relation = _b(sub[1]), _b(sub[2]), _b(sub[3])
    return m


def response_message(tuples, token=""):
    m = ListResponseMsg()
    for t in tuples:
        fill_tuple(m.relation_tuples.add(), t)
    m.next_page_token = _b(token)
    return m


def response_proto(tuples, token="") -> bytes:
    return response_message(tuples, token).SerializeToString(deterministic=True)


def response(encoding, tuples, token="") -> bytes:
    return response_json(tuples, token) if encoding in ("json", ENC_JSON) else response_proto(tuples, token)


# ---------------------------------------------------------------------------------------------
# The escape table: every class of go_json_string, one string each (and a few neighbours that must
# stay as they are).
ESCAPE_CASES = [
    b'"', b"\\", b"\n", b"\r", b"\t", b"\x08", b"\x0c", b"\x00", b"\x01", b"\x1f", b" ", b"\x7f", b"<", b">", b"&",
    b"/", b"'", "\u2028".encode(), "\u2029".encode(), "\u2027".encode(), "\u202a".encode(),
    "é".encode(), "€".encode(), "\U0001F600".encode(), "\U0010FFFF".encode(),
    b"\xc3", b"\xc3(", b"a\xc3", b"\xc0\x80", b"\xe0\x80\x80", b"\xf0\x80\x80\x80", b"\xed\xa0\x80", b"\xed\x9f\xbf",
    b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"\x80", b"\xbf", b"\xff", b"\xe2\x82", b"\xf0\x9f\x98",
    b"", b"plain", b'a"b\\c\nd<e>f&g\xc3h\xe2\x80\xa8i',
]

# A fixed one-to-one renaming of tests/randgraph.py's objects and users (relations keep their names)
# onto strings that hold every escape class.  "" is only possible for a subject id (a tuple with an
# empty object cannot be stored: the store reads it as a wildcard).
RENAME = {
    "a": b'q"uote', "b": b"back\\slash", "c": b"line\nfeed\ttab", "d": b"ctl\x01del\x7f", "a#b": b"<html>&amp;",
    "B": "sep\u2028para\u2029".encode(), "é": "é€\U0001F600".encode(),
    "u": b"lone\xc3", "v": b"over\xc0\x80long", "w": b"sur\xed\xa0\x80rogate", "U": b"",
}


def rename(s: str) -> bytes:
    """The renamed string; names outside the table (randgraph's users of the form ns:obj#rel, the
    relations) keep theirs, which no renamed string equals."""
    return RENAME[s] if s in RENAME else s.encode()


def sql_text(b: bytes) -> str:
    return b.decode("latin-1")


def raw_bytes(s: str) -> bytes:
    return s.encode("latin-1")


def _rt(s: str) -> str:
    return sql_text(rename(s))


def renamed_store(seed, **kw):
    """tests/randgraph.random_store with RENAME applied before anything is built ->
    (SQLite store over the Latin-1 text, namespaces, snapshot rows holding the bytes, page size,
    (names, objects, relations, users) as the text the store holds)."""
    namespaces, tuples, raw, ps, (names, objs, rels, users) = random_graph(seed, **kw)

    def sub(s):
        return SubjectID(_rt(s.id)) if isinstance(s, SubjectID) else SubjectSet(s.namespace, _rt(s.object) if s.object else "", s.relation)
    tuples = [RelationTuple(t.namespace, _rt(t.object), t.relation, sub(t.subject)) for t in tuples]
    raw = [(n, _rt(o), r, None if sid is None else _rt(sid), sns, None if so is None else _rt(so), sr)
           for n, o, r, sid, sns, so, sr in raw]
    store = SQLStore(namespaces, tuples, page_size=ps, raw_rows=raw)
    from tests.engine_util import rows_from_tuples
    rows = [tuple(raw_bytes(x) if isinstance(x, str) else x for x in row) for row in rows_from_tuples(namespaces, tuples, raw)]
    return store, namespaces, rows, tuples, raw, ps, (names, [_rt(o) for o in objs], rels, [_rt(u) for u in users])


def key_bytes(k):
    """A list_util.tuple_key over the store's text -> the same tuple over the bytes."""
    ns, obj, rel, sub = k
    return (raw_bytes(ns), raw_bytes(obj), raw_bytes(rel), (sub[0],) + tuple(raw_bytes(x) for x in sub[1:]))


def request_bytes(q):
    """A list_util query over the store's text -> the tuple Snapshot.list_encode takes, over the bytes."""
    ns, obj, rel, sub, size, page = list_util.to_request(q)
    if sub is not None:
        sub = (sub[0],) + tuple(raw_bytes(x) for x in sub[1:])
    return (raw_bytes(ns), raw_bytes(obj), raw_bytes(rel), sub, size, page)


def expected_body(store, query, encoding):
    """(status, body, token, total, n_tuples) as Snapshot.list_encode reports an answered query."""
    status, keys, token, total = list_util.expected(store, query)
    if status != list_util.LIST_OK:
        return (status, b"", "", 0, 0)
    return (status, response(encoding, [key_bytes(k) for k in keys], token), token, total, len(keys))
