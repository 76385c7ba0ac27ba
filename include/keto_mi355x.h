/*
 * keto_mi355x.h -- C-ABI of the MI355X batched check / expand engine.
 *
 * This is the drop-in boundary for Keto's read hot path.  Each entry point replaces one
 * reference interface (paths relative to the reference tree, icyphox/keto = ory/keto v0.8.1):
 *
 *   keto_snapshot_build      replaces the per-node SQL reads the engines issue through
 *                            relationtuple.Manager.GetRelationTuples
 *                            (internal/relationtuple/definitions.go:29;
 *                             internal/persistence/sql/relationtuples.go:238-277) with one
 *                            immutable CSR snapshot built from a full scan of keto_relation_tuples
 *                            in the same ORDER BY (relationtuples.go:250).
 *   keto_check_batch         replaces check.(*Engine).SubjectIsAllowed
 *                            (internal/check/engine.go:116-123), batched.
 *   keto_expand_batch        replaces expand.(*Engine).BuildTree
 *                            (internal/expand/engine.go:33-102), batched.
 *   keto_tree_*              replace the expand.Tree value and its JSON codec
 *                            (internal/expand/tree.go:26-30,156-163).
 *
 * All strings are borrowed (keto_str = pointer + length, not NUL-terminated) and only read
 * during the call.  The library keeps no caller pointers after a call returns.  A snapshot may be
 * shared by concurrent *_batch calls from any threads; calls on one snapshot run one at a time on its
 * device (a batch's persistent grid fills the whole GPU, so overlapping two would not finish either
 * sooner), each call's host-side work (resolution, staging) runs in the calling thread.  The
 * exception is keto_check_batch_packed with a small batch (below), whose calls from several threads
 * keep up to KETO_PACKED_SLOTS (default 2) batches in flight: one's upload and resolution run while
 * another's check does.
 * Every call returns KETO_OK (0) or a negative KETO_E_* code; keto_last_error() then holds a
 * thread-local message.  There is no CPU fallback inside the library: when the HIP runtime or a
 * device is missing, compute calls fail with KETO_E_HIP.
 */
#ifndef KETO_MI355X_H
#define KETO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KETO_ABI_VERSION 8
/* The largest arena one snapshot (a replica) or one partition part takes on a device: handles are
 * 32-bit; below 2^31 a count of 16-byte units (subject-set targets, and the root rows of the first
 * 32 GiB), above it a count of 32-, 64- or 128-byte units of the root rows past 32 GiB (arenas past
 * 64 GiB, whatever unit gives every root row a handle).  A graph past it is served as several
 * shared-rows parts, more than one per device if need be (each part holds the subject-set targets and
 * its share of the root rows).  Targets alone are capped at 32 GiB. */
#define KETO_ARENA_MAX_BYTES (288ull << 30)

/* return codes */
#define KETO_OK 0
#define KETO_E_INVALID (-1)     /* bad argument */
#define KETO_E_HIP (-2)         /* HIP runtime / device error, or no device */
#define KETO_E_NOMEM (-3)       /* host or device allocation failed */
#define KETO_E_CONFIG (-4)      /* namespace config not supported (duplicate ids or names) */
#define KETO_E_RANGE (-5)       /* a size limit of the snapshot format was exceeded */
#define KETO_E_REBUILD (-6)     /* keto_snapshot_apply: this write needs a rebuild (snapshot unchanged) */

/* per-query status of keto_check_batch (allowed_out is always valid) */
#define KETO_CHECK_OK 0                 /* decision equals the reference engine's */
#define KETO_CHECK_UNKNOWN_NAMESPACE 1  /* request namespace unknown: reference returns false (engine.go:98-100) */
#define KETO_CHECK_UNDECIDED 2          /* no tier could decide it within the engine's limits (allowed_out = 0):
                                           ask the reference engine; the other requests of
                                           the batch are decided as usual */

/* decision byte of the ids / device entry points: 0 = denied, 1 = allowed, KETO_UNDECIDED = the
 * request exceeded the engine's limits on its final tier (per request, never the whole batch) */
#define KETO_UNDECIDED 2

/* per-root status of keto_expand_batch */
#define KETO_EXPAND_TREE 0              /* a tree (BuildTree returned a non-nil *Tree) */
#define KETO_EXPAND_NIL 1               /* BuildTree returned nil, nil (JSON null) */
#define KETO_EXPAND_NOT_FOUND 2         /* BuildTree returned herodot.ErrNotFound (unknown namespace, A.Q8/Q9) */
#define KETO_EXPAND_UNDECIDED 3         /* the tree exceeded the engine's limits: ask the reference engine */

/* node types of an expand tree (internal/expand/tree.go:16-23; only union and leaf are produced) */
#define KETO_NODE_UNION 0
#define KETO_NODE_LEAF 1

typedef struct {
    const char* p;
    uint32_t n;
} keto_str;

/* namespace.Namespace{ID, Name} (internal/namespace/definitions.go:9-13), in config order */
typedef struct {
    int32_t id;
    keto_str name;
} keto_namespace;

/* one row of keto_relation_tuples (internal/persistence/sql/relationtuples.go:19-31).
 * Array order = commit order (commit_time ties are broken by position). */
typedef struct {
    int32_t namespace_id;
    keto_str object;
    keto_str relation;
    uint8_t subject_kind;       /* 0 = subject_id, 1 = subject set */
    keto_str subject_id;        /* kind 0 */
    int32_t set_namespace_id;   /* kind 1 */
    keto_str set_object;        /* kind 1 */
    keto_str set_relation;      /* kind 1 */
} keto_tuple;

/* a Subject by name (internal/relationtuple/definitions.go:77-117) */
typedef struct {
    uint8_t kind;               /* 0 = SubjectID, 1 = SubjectSet */
    keto_str id;                /* kind 0 */
    keto_str set_namespace;     /* kind 1 */
    keto_str set_object;
    keto_str set_relation;
} keto_subject;

/* check request = InternalRelationTuple + request max-depth (CheckRequest, check_service.proto) */
typedef struct {
    keto_str namespace_;
    keto_str object;
    keto_str relation;
    keto_subject subject;
    int32_t max_depth;          /* <= 0 or > global -> global (engine.go:118-120) */
} keto_check_req;

/* pre-resolved check request (keto_resolve_checks), 16 bytes; the form the device consumes.
 * Rows are named by *row handles* (their place in the device arena; keto_row_handles maps row ids,
 * i.e. positions in (namespace_id, object, relation) order, to handles). */
typedef struct {
    uint32_t row;               /* top-level row handle, or KETO_NO_ROW */
    uint32_t target;            /* subject: ID string id, or row handle of a subject set, or KETO_NO_TARGET */
    uint32_t flags;             /* bit0: target is a subject set */
    int32_t max_depth;          /* request max-depth (clamped on the device) */
} keto_check_ids;
#define KETO_NO_ROW 0xFFFFFFFFu
#define KETO_NO_TARGET 0xFFFFFFFFu

/* expand request (ExpandRequest, expand_service.proto) */
typedef struct {
    keto_subject subject;
    int32_t max_depth;
} keto_expand_req;

/* one node of an expand tree in pre-order.  subject: bit31 set -> subject set (bits 0..30 = row
 * id), else subject id (bits 0..30 = string id).  info: bit31 set -> leaf, bits 0..30 = number of
 * children (all children follow in pre-order). */
typedef struct {
    uint32_t subject;
    uint32_t info;
} keto_tree_node;

typedef struct {
    uint32_t page_size;         /* 0 -> 100 (internal/persistence/sql/persister.go:46) */
    int32_t device;             /* HIP device ordinal; -1 = host-only snapshot (no compute) */
    uint32_t flags;             /* reserved, 0 */
} keto_snapshot_opts;

typedef struct keto_snapshot keto_snapshot;
typedef struct keto_tree_arena keto_tree_arena;

typedef struct {
    uint64_t n_tuples;
    uint64_t n_edges;           /* including materialized wildcard rows */
    uint32_t n_rows;            /* real + empty + wildcard rows */
    uint32_t n_real_rows;
    uint32_t n_wildcard_rows;
    uint32_t n_seq_rows;        /* rows on the ordered (collision / wildcard) path */
    uint32_t n_poisoned_rows;
    uint32_t n_strings;
    uint32_t n_collision_keys;
    uint64_t device_bytes;
} keto_snapshot_stats;

int keto_abi_version(void);
const char* keto_last_error(void);

/* Build a snapshot from the tuple table; sorts with the reference ORDER BY itself. */
int keto_snapshot_build(const keto_namespace* namespaces, uint32_t n_namespaces, const keto_tuple* tuples,
                        uint64_t n_tuples, const keto_snapshot_opts* opts, keto_snapshot** out);

/* Bulk loader for pre-interned, pre-ordered data (synthetic / exported snapshots).
 * row_ns/row_obj/row_rel: per row, namespace id and string ids; rows must be in
 * (namespace_id, object bytes, relation bytes) order.  row_ptr: n_rows+1 offsets into edges.
 * edges: per row, subject sets first (bit31 set, bits 0..30 = target row) in reference order, then
 * subject ids (bits 0..30 = string id) in byte order.  strings: n_strings strings in byte order
 * (string id = index).  The caller guarantees that no Subject.String() of two different subjects
 * coincide and that every subject set resolves to a row (pass empty rows for dangling sets). */
int keto_snapshot_from_csr(const keto_namespace* namespaces, uint32_t n_namespaces, uint32_t n_rows,
                           const int32_t* row_ns, const uint32_t* row_obj, const uint32_t* row_rel,
                           const uint64_t* row_ptr, const uint32_t* edges, const keto_str* strings,
                           uint32_t n_strings, const keto_snapshot_opts* opts, keto_snapshot** out);

void keto_snapshot_release(keto_snapshot* s);

/* A replica of an unpartitioned snapshot for another device (device = -1: host only), at the source's
 * current version, without scanning or sorting the table again: the host tables are copied and laid
 * out afresh, then uploaded.  One server process serving the node's GPUs keeps one replica per
 * device, deals batches among them and applies every write transaction to each (the reference serves
 * every request from one process, internal/driver/daemon.go:62-69, on engines built once per registry,
 * internal/driver/registry_default.go:159-171).  Replicas are independent snapshots afterwards. */
int keto_snapshot_clone(const keto_snapshot* src, int32_t device, keto_snapshot** out);

/* Persisted snapshot (the optional on-disk CSR): keto_snapshot_save writes the
 * host tables of an unpartitioned snapshot at its current version (the interned strings, the rows in
 * ORDER BY order with their page cuts and edges, the collision classes, the rows writes changed) to
 * `path` (through <path>.tmp and a rename, so an interrupted save leaves an older file intact), with
 * the caller's 64-bit `tag` -- e.g. the table's last commit covered, so that a restarting server
 * replays only later transactions (the reference re-reads the table on every query,
 * internal/persistence/sql/relationtuples.go:249-251; a GPU server otherwise rebuilds the snapshot
 * from a full scan and sort).  keto_snapshot_load reads it back, lays it out and uploads it to
 * `device` (-1: host only); *tag_out (may be NULL) gets the tag.  The loaded snapshot answers every
 * call exactly as the saved one did and has its version.  A file that is not a snapshot, has another
 * format, is truncated or fails a section checksum: KETO_E_INVALID. */
int keto_snapshot_save(const keto_snapshot* s, const char* path, uint64_t tag);
int keto_snapshot_load(const char* path, int32_t device, keto_snapshot** out, uint64_t* tag_out);

/* Snapshot lifecycle: apply one write transaction the way TransactRelationTuples does
 * (internal/persistence/sql/relationtuples.go:289-297): the inserts first (each after every equal
 * tuple, as commit_time orders them, :128-149), then the deletes (every tuple equal in namespace,
 * object, relation and subject, :200-223).  The changed rows are rewritten in the device arena in
 * place (forwards when a row outgrows its place; the tail grows on demand) and closure filters are
 * re-closed, between batches; later batches see the new version.  New Subject.String() collisions
 * (collision classes, ROW_SEQ rows) and stored subject sets with an empty field (their materialized
 * rows, re-materialized when a row they match changes) are patched in place too.  A part of an
 * edge-partitioned snapshot (KETO_PART_SHARED) takes every transaction and writes the rows it holds;
 * a migrating part takes none (KETO_E_INVALID).  An unknown namespace id fails the whole transaction
 * (KETO_E_INVALID), like GetNamespaceByName.  KETO_E_REBUILD: the write touches a poisoned row (a
 * tuple of an unconfigured namespace) or a wildcard row that matches one; the snapshot is unchanged
 * and the caller rebuilds it from the table.  Row handles (keto_row_handles,
 * keto_resolve_checks) are per version: resolve again after a write.  *version_out (may be NULL)
 * gets the new version: the snaptoken the reference leaves "not yet implemented"
 * (internal/check/handler.go:182). */
int keto_snapshot_apply(keto_snapshot* s, const keto_tuple* inserts, uint64_t n_inserts, const keto_tuple* deletes,
                        uint64_t n_deletes, uint64_t* version_out);
/* Version of the snapshot: 0 after the build, +1 per keto_snapshot_apply or keto_snapshot_delete_query. */
uint64_t keto_snapshot_version(const keto_snapshot* s);

/* Edge-partitioned upload, for graphs larger than one GPU (one process per GPU, n_parts parts).
 * Takes a host-only snapshot (built with device = -1) and uploads to `device` only
 *   - every row that is the target of some subject set (these are kept on all parts), and
 *   - the root rows (rows no subject set points at) whose hash(namespace_id, object) % n_parts
 *     == part.
 * A check or expand whose top-level row is a root row must run on the part keto_row_owner names
 * (requests are routed with one all-to-all; see keto_amd/multi.py); the traversal below the top
 * level only visits rows every part holds, so each part answers exactly.  Calls naming another
 * part's root row fail with KETO_E_INVALID.  Replaces nothing in the reference. */
int keto_snapshot_upload_part(keto_snapshot* s, uint32_t part, uint32_t n_parts, int32_t device);

/* Partition modes of keto_snapshot_upload_part_mode. */
#define KETO_PART_SHARED 0      /* keto_snapshot_upload_part: set targets on every part, root rows by hash */
#define KETO_PART_MIGRATE 1     /* every row on exactly one part by hash(namespace_id, object) */
#define KETO_MIG_MAX_PARTS 30
/* Edge-partitioned upload in either mode.  KETO_PART_MIGRATE is for graphs whose set-target rows
 * (folders, groups) do not fit on one GPU either: each part holds only its own rows, plus a stub for
 * every other part's row one of its subject sets points at, and a check's DFS migrates between parts
 * at those crossings (keto_mig_begin / keto_mig_round).  After the upload the parts exchange closure
 * filters (keto_part_stubs / keto_part_filters / keto_part_close) until no filter changes anywhere,
 * then call keto_part_closure_done.  A migrating part answers checks only through keto_mig_*;
 * expand and the other check entry points fail with KETO_E_INVALID.  n_parts <= 30. */
int keto_snapshot_upload_part_mode(keto_snapshot* s, uint32_t part, uint32_t n_parts, int32_t device, uint32_t mode);
/* KETO_PART_MIGRATE with the rows most subject sets point at (the hottest in-degree bands whose rows
 * fit hot_bytes of arena) replicated on every part, at the same place: searches cross parts only on
 * the colder rows.  hot_bytes = 0 is keto_snapshot_upload_part_mode(..., KETO_PART_MIGRATE); every
 * part of one partition must be uploaded with the same hot_bytes. */
int keto_snapshot_upload_part_migrate(keto_snapshot* s, uint32_t part, uint32_t n_parts, int32_t device,
                                      uint64_t hot_bytes);
/* Arena a part of an edge-partitioned upload would hold (host-only snapshots; sizing aid):
 * arena_bytes of the part's device arena, shared_bytes of it in rows every part keeps. */
typedef struct {
    uint64_t arena_bytes;
    uint64_t shared_bytes;
    uint32_t rows;              /* rows on the part (stubs not counted) */
    uint32_t shared_rows;       /* of them: rows on every part (KETO_PART_SHARED: set targets; KETO_PART_MIGRATE:
                                   the replicated hot rows, shared_bytes their arena) */
    uint32_t root_rows;         /* of them: this part's root rows */
    uint64_t stub_rows;         /* KETO_PART_MIGRATE: stubs of other parts' rows */
} keto_part_stats;
int keto_snapshot_part_stats(keto_snapshot* s, uint32_t part, uint32_t n_parts, keto_part_stats* out);
int keto_snapshot_part_stats_mode(keto_snapshot* s, uint32_t part, uint32_t n_parts, uint32_t mode,
                                  keto_part_stats* out);

/* Closure-filter exchange of a migrating partition.  A closure filter (KETO_FILTER_WORDS words) is
 * the bloom filter of every subject id reachable from a row; a stub must carry its row's filter from
 * the owner part.  Round: every part lists its stubs (keto_part_stubs: row ids, ascending; returns
 * the count, writes at most cap), asks each stub's owner (keto_row_owner) for its current filter
 * (keto_part_filters on the owner: the filters of rows it holds, stubs included), and ORs the answers into its stubs
 * (keto_part_close, which then re-closes the part's own filters; *changed_out = filters that
 * changed).  When a round changes nothing on any part, every filter is exact: keto_part_closure_done
 * (converged = 1).  converged = 0 gives all-ones filters (no pruning; still exact answers). */
#define KETO_FILTER_WORDS 22
int64_t keto_part_stubs(const keto_snapshot* s, uint32_t* rows_out, uint64_t cap);
int keto_part_filters(keto_snapshot* s, const uint32_t* rows, uint64_t n, uint32_t* filters_out);
int keto_part_close(keto_snapshot* s, const uint32_t* stub_rows, uint64_t n, const uint32_t* filters,
                    uint64_t* changed_out);
int keto_part_closure_done(keto_snapshot* s, int converged);

/* Check batches on a migrating partition (replaces check.(*Engine).SubjectIsAllowed,
 * internal/check/engine.go:116-123, for graphs spread over several GPUs).  keto_mig_begin takes the
 * requests routed to this part (row-id form, every top-level row owned here: keto_row_owner /
 * keto_route_rows_device) and runs their searches until each is decided or crosses to another
 * part.  The crossings come back as continuation records grouped by destination part (out->units[p]
 * 16-B units at d_records + the prefix of units before p, out->records[p] records whose unit
 * offsets inside p's segment are at d_offsets + the prefix of records before p; valid until the next
 * call on this snapshot).  The caller exchanges them (one all-to-all: each part receives the
 * segments addressed to it from every source part, concatenated in source order) and passes what it
 * received to keto_mig_round (in_records[s], in_units[s] per source part s), which continues the
 * searches and emits the next records.  Decisions land in d_allowed_out (the routed batch's order)
 * of the part that began the request.  The batch is done when a round emits no record on any part.
 * Decision bytes as keto_check_batch_device (KETO_UNDECIDED: a search beyond the engine's limits). */
typedef struct {
    uint64_t units[KETO_MIG_MAX_PARTS];
    uint32_t records[KETO_MIG_MAX_PARTS];
    const void* d_records;
    const uint32_t* d_offsets;
    uint32_t decided;           /* decisions written on this part in the call */
    uint32_t undecided;         /* of the searches ended in the call: KETO_UNDECIDED */
    uint32_t processed;         /* records (requests, continuations, decisions) handled in the call */
    uint32_t reruns;            /* of them: re-run with bigger visited tables or a bigger record pool */
} keto_mig_out;
int keto_mig_begin(keto_snapshot* s, const keto_check_ids* d_reqs, uint32_t n, int32_t global_max_depth,
                   uint8_t* d_allowed_out, void* stream, keto_mig_out* out);
int keto_mig_round(keto_snapshot* s, const void* d_records, const uint32_t* d_offsets, const uint32_t* in_records,
                   const uint64_t* in_units, void* stream, keto_mig_out* out);
/* Free and total device memory of HIP device `device` (hipMemGetInfo): the Go server sizes its
 * placement with it -- replicas while the replicated arena (keto_snapshot_part_stats_mode with
 * n_parts = 1) and the engine's workspaces fit every device, else shared-rows parts over the devices
 * (the reference serves any table size from one process, internal/driver/daemon.go:62-69). */
int keto_device_memory(int32_t device, uint64_t* free_out, uint64_t* total_out);
/* Device-to-device copy on `stream`, returning when it is done: for callers whose exchange layer
 * needs the records in buffers of its own (e.g. torch.distributed tensors). */
int keto_device_copy(void* dst, const void* src, uint64_t bytes, void* stream);
/* keto_check_batch_device on requests that name rows by row id (row and subject-set target), the
 * form requests travel in between parts: each is translated to this device's handles first.  A
 * request for another part's root row fails the call with KETO_E_INVALID. */
int keto_check_batch_rows_device(keto_snapshot* s, const keto_check_ids* d_reqs, uint32_t n, int32_t global_max_depth,
                                 uint8_t* d_allowed_out, void* stream);
/* Owner part of each row id for n_parts parts: -1 = a row every part holds (route anywhere; a
 * KETO_PART_SHARED part's set targets).  A KETO_PART_MIGRATE part owns every row it holds. */
int keto_row_owner(const keto_snapshot* s, const uint32_t* rows, uint64_t n, uint32_t n_parts, int32_t* out);
/* Device-side routing of a row-id batch over n_parts (<= 64) parts, all buffers on one device:
 * a stable counting sort by destination part = d_owner[row] (keto_row_owner's output as int16,
 * n_rows entries), or self_part for rows every part holds, KETO_NO_ROW and out-of-range rows (the
 * destination's keto_check_batch_rows_device then rejects the latter).  Writes d_send (the n
 * requests grouped by part, batch order kept inside each part), d_order (batch index of each
 * d_send entry) and counts_out[n_parts] (host: requests per part, the all-to-all split sizes).
 * d_work: keto_route_work_bytes(n, n_parts) bytes of device scratch.  Synchronizes `stream`.
 * Replaces the host-side grouping of a partitioned batch (repo:keto_amd/multi.py). */
uint64_t keto_route_work_bytes(uint32_t n, uint32_t n_parts);
int keto_route_rows_device(const keto_check_ids* d_reqs, uint32_t n, const int16_t* d_owner, uint32_t n_rows,
                           uint32_t self_part, uint32_t n_parts, void* d_work, uint64_t work_bytes,
                           keto_check_ids* d_send, uint32_t* d_order, uint32_t* counts_out, void* stream);
/* Inverse of the routing for the decisions: d_out[d_order[j]] = d_back[j] for j < n (enqueued on
 * `stream`). */
int keto_unroute_device(const uint8_t* d_back, const uint32_t* d_order, uint32_t n, uint8_t* d_out, void* stream);
int keto_snapshot_get_stats(const keto_snapshot* s, keto_snapshot_stats* out);

/* Row ids (snapshot row order; KETO_NO_ROW passes through) -> row handles for keto_check_ids. */
int keto_row_handles(const keto_snapshot* s, const uint32_t* rows, uint64_t n, uint32_t* out);

/* Resolve named requests to device form; status_out gets KETO_CHECK_* (may be NULL). */
int keto_resolve_checks(const keto_snapshot* s, const keto_check_req* reqs, uint32_t n, keto_check_ids* out,
                        uint8_t* status_out);

/* Batched SubjectIsAllowed.  allowed_out[i] = 0/1, status_out[i] = KETO_CHECK_* (may be NULL). */
int keto_check_batch(keto_snapshot* s, const keto_check_req* reqs, uint32_t n, int32_t global_max_depth,
                     uint8_t* allowed_out, uint8_t* status_out);

/* Check requests with their strings packed back to back in one buffer, resolved on the GPU.  Request
 * i's fields start at blob + reqs[i].off: namespace, object, relation, then the subject id (kind 0)
 * or the subject set's namespace, object and relation (kind 1), with their byte lengths in
 * reqs[i].len -- the form a caller that already copies a batch's strings into one arena (the Go
 * batcher's C memory) hands over without building keto_check_req structs.  The library copies blob
 * and records to the device and resolves every request there against the snapshot's string and row
 * indexes (whereQuery, internal/persistence/sql/relationtuples.go:178-198; the indexes are uploaded
 * once per snapshot version), then checks them (check.(*Engine).SubjectIsAllowed,
 * internal/check/engine.go:116-123): decisions and statuses equal keto_check_batch's on the same
 * requests.  Requests with an empty namespace, object or relation (wildcard queries, in the subject
 * set too) are resolved on the host as keto_check_batch does.  blob_len < 2^32; fields of up to
 * 65535 bytes (longer ones: keto_check_batch).  A request whose fields lie outside the blob fails the
 * call (KETO_E_INVALID, naming the first such request) before anything is written to the outputs.
 * Large batches are pipelined (pieces of KETO_PACKED_CHUNK requests, default 2^21, uploaded while
 * earlier pieces are resolved and checked): fastest when the strings are packed in request order, as
 * the Go batcher packs them; any other layout gives the same answers after a second pass.  Pinned
 * blob and records (keto_host_alloc) let the upload run asynchronously. */
typedef struct {
    uint32_t off;               /* byte offset of the request's first field in blob */
    uint16_t len[6];            /* namespace, object, relation, subject id | set namespace, set object, set relation */
    uint8_t kind;               /* 0 = subject id (len[0..3]), 1 = subject set (len[0..5]) */
    uint8_t reserved;
    int32_t max_depth;          /* <= 0 or > global -> global (engine.go:118-120) */
} keto_check_packed;
int keto_check_batch_packed(keto_snapshot* s, const char* blob, uint64_t blob_len, const keto_check_packed* reqs,
                            uint32_t n, int32_t global_max_depth, uint8_t* allowed_out, uint8_t* status_out);

/* Same with pre-resolved requests in host memory (decision bytes as above, KETO_UNDECIDED
 * included).  Host-buffer calls run as a pipeline of chunks: the H2D copy of the next chunk and the
 * D2H copy of the previous one overlap the check of the current one.  Buffers from keto_host_alloc
 * (pinned) are copied directly; pageable ones go through the library's pinned staging. */
int keto_check_batch_ids(keto_snapshot* s, const keto_check_ids* reqs, uint32_t n, int32_t global_max_depth,
                         uint8_t* allowed_out);

/* Same with requests that name rows by row id (row, and subject-set targets): the form a caller
 * that interned names once keeps (snapshot row order, keto_row_handles' input).  Translated to
 * device handles on the device, inside the pipeline. */
int keto_check_batch_rows(keto_snapshot* s, const keto_check_ids* reqs, uint32_t n, int32_t global_max_depth,
                          uint8_t* allowed_out);

/* Compact 8-byte request of keto_check_batch_pairs: the top-level row by row id, and the subject:
 * bit31 set -> a subject set (bits 0..30 = its row id), else a subject-id string id;
 * KETO_NO_TARGET = a subject the snapshot does not know. */
typedef struct {
    uint32_t row;
    uint32_t subject;
} keto_check_pair;

/* keto_check_batch_rows for batches whose requests share one request max-depth (the usual case:
 * CheckRequest.max_depth unset -> 0 -> the global maximum): half the PCIe bytes per request. */
int keto_check_batch_pairs(keto_snapshot* s, const keto_check_pair* reqs, uint32_t n, int32_t max_depth,
                           int32_t global_max_depth, uint8_t* allowed_out);

/* Pinned (page-locked) host memory for request / decision buffers of the host-buffer calls. */
int keto_host_alloc(uint64_t bytes, void** out);
void keto_host_free(void* p);

/* Same with requests and results resident in device memory of the snapshot's device; enqueued on
 * `stream` (a hipStream_t, NULL = default stream).  Returns after enqueueing; results are ready
 * when the stream is synchronized. */
int keto_check_batch_device(keto_snapshot* s, const keto_check_ids* d_reqs, uint32_t n, int32_t global_max_depth,
                            uint8_t* d_allowed_out, void* stream);

/* ---- Multi-GPU: communicators (repo:keto_amd/csrc/comm.cpp) ----
 * The exchanges of SURVEY.md 8(e) inside the library, for callers without Python (the Go server
 * process, internal/driver/daemon.go:62-69, calling check.(*Engine).SubjectIsAllowed per request,
 * internal/check/engine.go:116-123).  Every call below taking a keto_comm is collective: all ranks of
 * the communicator call it.  Errors are agreed: a rank whose own part fails (a bad argument, a
 * request it cannot route, an allocation or kernel error) still takes part in the status exchange
 * that precedes every data exchange, and every rank then returns the same code (that of the lowest
 * failing rank; keto_last_error says which rank failed), so a local error never leaves the peers
 * waiting.  Only a failing transport (RCCL, or a local rank that does not arrive within
 * KETO_COMM_TIMEOUT_MS, default 600000) returns KETO_E_HIP without agreement.
 *
 * Two transports:
 *   keto_comm_init        one process per GPU over RCCL (xGMI).  keto_comm_id makes a communicator id
 *                         on one rank; the caller hands its KETO_COMM_ID_BYTES to every rank (its own
 *                         channel), and every rank calls keto_comm_init with it.
 *   keto_comm_init_local  the ranks are threads of ONE process (one server process driving several
 *                         GPUs, or several parts on one GPU), each rank's calls made from its own
 *                         thread; the exchanges are device copies (peer copies between GPUs).  The id
 *                         is any KETO_COMM_ID_BYTES the caller chooses (the same for every rank of the
 *                         communicator, unique among the process's live local communicators). */
#define KETO_COMM_ID_BYTES 128
typedef struct keto_comm keto_comm;
int keto_comm_id(uint8_t* id_out);
int keto_comm_init(const uint8_t* id, int32_t n_ranks, int32_t rank, int32_t device, keto_comm** out);
int keto_comm_init_local(const uint8_t* id, int32_t n_ranks, int32_t rank, int32_t device, keto_comm** out);
void keto_comm_free(keto_comm* c);
/* Replicated snapshot (every rank uploaded the whole graph): every rank passes the same n named
 * requests (keto_check_batch's form); rank r decides the r-th contiguous shard, and one all-gather
 * returns all n decisions and statuses to every rank. */
int keto_check_batch_sharded(keto_comm* c, keto_snapshot* s, const keto_check_req* reqs, uint32_t n,
                             int32_t global_max_depth, uint8_t* allowed_out, uint8_t* status_out);
/* Edge-partitioned snapshot (this rank's part: keto_snapshot_upload_part_mode with part = rank and
 * n_parts = ranks): every rank passes its own batch; requests go to the parts owning their rows
 * (one all-to-all), are decided there -- on a migrating part by continuation-record rounds with an
 * all-reduce and all-to-alls per round -- and the decisions come back (a second all-to-all).  A
 * wildcard query that no stored subject set uses has no row to route by: a shared-rows part answers
 * it itself (its batch-local row from the whole graph's host tables); a migrating part sends one
 * request per matching row (each top-level tuple is searched with a fresh visited map, so the query
 * is allowed iff one of those rows is); when a page of the query's ORDER BY sequence fails, the rows
 * before that page go whole and the row it cuts one top-level tuple at a time (relationtuples.go:
 * 64-71; engine.go:98-100).  Every rank returns the same code when any rank fails. */
int keto_check_batch_routed(keto_comm* c, keto_snapshot* s, const keto_check_req* reqs, uint32_t n,
                            int32_t global_max_depth, uint8_t* allowed_out, uint8_t* status_out);
/* The same for a packed batch (the keto_check_batch_packed layout: strings back to back in
 * blob, one keto_check_packed record per request), resolved on this rank's device instead of on
 * host threads (ABI 6): the partitioned form of the Go shim's CheckBatch
 * (integration/go/internal/gpu/partition.go).  Decisions, statuses and errors as
 * keto_check_batch_routed; a request whose fields lie outside the blob fails the call on every rank. */
int keto_check_batch_routed_packed(keto_comm* c, keto_snapshot* s, const char* blob, uint64_t blob_len,
                                   const keto_check_packed* reqs, uint32_t n, int32_t global_max_depth,
                                   uint8_t* allowed_out, uint8_t* status_out);
/* BuildTree (internal/expand/engine.go:33-102) over an edge-partitioned snapshot of shared-rows
 * parts (KETO_PART_SHARED; this rank's part as above): every rank passes its own roots; a root row
 * another part owns is expanded on that part (one all-to-all of roots, one of trees), every other
 * root here, as keto_expand_batch does.  *out: one arena in request order, read with keto_tree_*
 * against this rank's snapshot.  A migrating part (KETO_PART_MIGRATE) expands every root itself: the
 * other parts' rows its trees reach are copied into the call's overlay from the host tables (which
 * every part holds whole) in rounds of the count pass; nothing is routed.  Errors are agreed as above. */
int keto_expand_batch_routed(keto_comm* c, keto_snapshot* s, const keto_expand_req* reqs, uint32_t n,
                             int32_t global_max_depth, keto_tree_arena** out);
/* A migrating partition's closure-filter exchange, once after every rank uploaded its part (before
 * the first keto_check_batch_routed; replaces the keto_part_filters / keto_part_close /
 * keto_part_closure_done loop a caller would otherwise run). */
int keto_comm_close_filters(keto_comm* c, keto_snapshot* s, uint32_t* rounds_out);

/* Device time of the last keto_check_* call on this snapshot, per tier (tier 0 = every request,
 * tiers 1/2 = requests whose visited map outgrew the previous tier's table), from HIP events on
 * the call's stream; summed over the chunks of a host-buffer call. */
typedef struct {
    float tier_ms[3];
    uint32_t requests[3];
    uint32_t undecided;         /* requests left KETO_UNDECIDED */
    uint32_t chunks;            /* host-buffer calls: pipeline chunks (0 for device calls) */
    float wall_ms;              /* host-buffer calls: entry to return, H2D + checks + D2H */
    float resolve_ms;           /* keto_check_batch: name resolution on host threads before the device part */
    float items_ms;             /* deep batches (max-depth > 9): top-level items split and pretested */
    uint32_t items;             /* deep batches: work requests (items + requests checked whole) */
    uint32_t items_kept;        /* deep batches: of them, checked after the reachability pretest */
    float index_ms;             /* deep batches: reverse / postings index (re)built for this snapshot version
                                   before the batch (host threads + upload; 0 when it was current) */
    uint32_t streamed;          /* pair batches from pinned memory: 1 = decided by the one streamed launch */
    uint32_t stream_stalls;     /* of the streamed launch: lanes whose wait for a chunk hit KETO_STREAM_WAIT_MS */
    uint32_t stream_fallbacks;  /* 1 = the streamed launch gave up (a stall) and the chunked pipeline decided */
} keto_batch_timing;
int keto_last_batch_timing(const keto_snapshot* s, keto_batch_timing* out);

/* Work counters of the traversal for a device-resident batch (instrumented kernels; same results):
 * out[0] row records read, out[1] subject-set edges scanned, out[2] subject-id words read by the
 * membership searches, out[3] visited-table probes, out[4] visited-table inserts, out[5] top-level
 * subject sets expanded (fresh visited maps).  Used for the roofline's algorithmic bytes.
 * out[6..12] are 128-B line touches per access stream (requests, row headers, edges, id tables,
 * id searches, frame pushes, frame pops): an upper bound of the kernel's L2 line traffic. */
#define KETO_WORK_SLOTS 16
/* Name of the tier-0 check kernel a batch at this global max-depth launches (as rocprofv3 prints
 * it, without the argument list), for matching profiles to bench lines.  Static storage. */
const char* keto_check_kernel_name(int32_t global_max_depth);
int keto_check_work_device(keto_snapshot* s, const keto_check_ids* d_reqs, uint32_t n, int32_t global_max_depth,
                           uint8_t* d_allowed_out, uint64_t out[KETO_WORK_SLOTS]);

/* Per-request loop iterations of the check_kernel tiers (deep batches, global max-depth > 9): the
 * length of each request's serial chain of dependent steps, for its latency histogram.  d_steps:
 * n uint32 on the device (instrumented kernels, same decisions). */
int keto_check_steps_device(keto_snapshot* s, const keto_check_ids* d_reqs, uint32_t n, int32_t global_max_depth,
                            uint8_t* d_allowed_out, uint32_t* d_steps);

/* Batched BuildTree.  The arena owns all trees; free it with keto_tree_arena_free.  Its node array
 * lives in page-locked host memory from a process-wide pool (blocks are recycled by later arenas;
 * up to 1 GiB of idle blocks is kept), so keto_tree_proto_all_device and
 * keto_tree_json_all_device upload it in one DMA. */
int keto_expand_batch(keto_snapshot* s, const keto_expand_req* reqs, uint32_t n, int32_t global_max_depth,
                      keto_tree_arena** out);
/* Same with pre-resolved roots: roots[i] bit31 set -> subject set (bits 0..30 = row id), else a
 * subject id (bits 0..30 = string id). */
int keto_expand_batch_ids(keto_snapshot* s, const uint32_t* roots, const int32_t* max_depth, uint32_t n,
                          int32_t global_max_depth, keto_tree_arena** out);
void keto_tree_arena_free(keto_tree_arena* a);
uint32_t keto_tree_count(const keto_tree_arena* a);
int keto_tree_status(const keto_tree_arena* a, uint32_t i);
/* pre-order nodes of tree i (NULL, *n = 0 for nil / error) */
const keto_tree_node* keto_tree_nodes(const keto_tree_arena* a, uint32_t i, uint64_t* n_nodes);
/* JSON of tree i exactly as Tree.MarshalJSON (internal/expand/tree.go:156-163); "null" for nil.
 * Writes at most cap bytes (NUL-terminated) and returns the full length, or a negative code. */
int64_t keto_tree_json(const keto_snapshot* s, const keto_tree_arena* a, uint32_t i, char* buf, uint64_t cap);
/* Every tree of the arena as JSON on host threads (the REST Expand response body of each root,
 * internal/expand/handler.go:77-91, h.d.Writer().Write of the
 * BuildTree result, via Tree.MarshalJSON): offsets[n+1], tree i = buf[offsets[i],
 * offsets[i+1]) -- keto_tree_json's text for a tree, "null" for a nil tree, empty for the roots
 * keto_tree_json reports as errors (KETO_EXPAND_NOT_FOUND / KETO_EXPAND_UNDECIDED).  buf is written
 * only if cap >= the total, which is returned (call with buf = NULL to size it).  A sizing call
 * keeps its encodings in the arena until the filling call (or keto_tree_arena_free), so the pair
 * encodes once; keto_tree_proto_all does the same. */
int64_t keto_tree_json_all(const keto_snapshot* s, const keto_tree_arena* a, char* buf, uint64_t cap,
                           uint64_t* offsets);

/* Tree i as acl.SubjectTree protobuf bytes, exactly as proto.Marshal(Tree.ToProto())
 * (internal/expand/tree.go:165-188; proto/ory/keto/acl/v1alpha1/expand_service.proto): the
 * gRPC Expand response's `tree`.  Writes min(cap, size) bytes, returns the size (0 for a nil tree,
 * which the reference sends as an unset field), or a negative code. */
int64_t keto_tree_proto(const keto_snapshot* s, const keto_tree_arena* a, uint32_t i, uint8_t* buf, uint64_t cap);
/* Every tree of the arena encoded on host threads: offsets[n+1] (tree i = buf[offsets[i],
 * offsets[i+1]), empty for nil / error trees); buf is written only if cap >= the total, which is
 * returned (call with buf = NULL to size it). */
int64_t keto_tree_proto_all(const keto_snapshot* s, const keto_tree_arena* a, uint8_t* buf, uint64_t cap,
                            uint64_t* offsets);
/* keto_tree_proto_all encoded on the GPU from the arena's nodes and the snapshot's strings (uploaded
 * to the snapshot's device on first use): the same bytes and offsets.  offsets
 * is always written; buf only when cap >= the returned total (call with buf = NULL to size it).
 * The call's device buffers stay with the snapshot for the next call (freed with its device
 * state); a pinned (hipHostMalloc'd) buf takes one DMA, a pageable one two pinned bounce chunks. */
int64_t keto_tree_proto_all_device(keto_snapshot* s, const keto_tree_arena* a, uint8_t* buf, uint64_t cap,
                                   uint64_t* offsets);
/* keto_tree_json_all encoded on the GPU the same way (the REST Expand response bodies, batched): the
 * same text and offsets -- keto_tree_json's text for a tree, "null" for a nil tree, empty for
 * KETO_EXPAND_NOT_FOUND / KETO_EXPAND_UNDECIDED roots, no NUL terminator.  offsets[n+1] is always
 * written; buf only when cap >= the returned total (call with buf = NULL to size it; unlike
 * keto_tree_json_all, nothing is kept between the sizing and the filling call).  Buffers as
 * keto_tree_proto_all_device: a pinned buf takes one DMA, a pageable one the two bounce chunks.
 * Fails like keto_tree_proto_all_device on a host-only snapshot (device = -1). */
int64_t keto_tree_json_all_device(keto_snapshot* s, const keto_tree_arena* a, char* buf, uint64_t cap,
                                  uint64_t* offsets);

/* Expand and encode in one call, the node arena never leaving the device: roots in, response bodies
 * out.  Replaces, for a batch, what the reference's Expand handlers do per request: BuildTree and
 * then h.d.Writer().Write(tree) via Tree.MarshalJSON (REST, internal/expand/handler.go:77-91,
 * internal/expand/tree.go:156-163), or BuildTree and then tree.ToProto() (gRPC,
 * internal/expand/handler.go:93-104, internal/expand/tree.go:165-188).  The bytes, offsets and
 * statuses are exactly those of keto_expand_batch[_ids] followed by keto_tree_status and
 * keto_tree_proto_all (KETO_ENC_PROTO) / keto_tree_json_all (KETO_ENC_JSON) on the same requests:
 * JSON has "null" for a nil tree and nothing for KETO_EXPAND_NOT_FOUND / KETO_EXPAND_UNDECIDED roots,
 * protobuf nothing for all three.  Against keto_expand_batch + a sizing and a filling
 * keto_tree_*_all_device call it saves the arena's D2H and H2D copies and the second run of the size
 * kernels: the trees are expanded into the snapshot's device buffers, their set handles and
 * batch-local wildcard rows turned into row ids by kernels there, sized once, written, and copied by
 * one DMA into a block of the library's pinned pool, which the result owns.
 * The result holds no reference to the snapshot: it stays readable after keto_snapshot_apply and
 * keto_snapshot_release, until keto_encoded_free.  n = 0 gives count 0, offsets {0} and total 0.
 * Errors: an unknown encoding is KETO_E_INVALID; a host-only snapshot (device = -1) and a root owned
 * by another shared-rows part fail as in keto_expand_batch (KETO_E_HIP / KETO_E_INVALID); a migrating
 * part (KETO_PART_MIGRATE, n_parts > 1) is KETO_E_INVALID -- it translates the rows it pulls from
 * other parts on the host: use keto_expand_batch and an encoder there.  keto_last_batch_timing
 * reports the expand passes as after keto_expand_batch. */
#define KETO_ENC_PROTO 0   /* acl.SubjectTree bytes, as keto_tree_proto_all */
#define KETO_ENC_JSON  1   /* Tree.MarshalJSON text, as keto_tree_json_all  */
typedef struct keto_encoded keto_encoded;
int keto_expand_encode_batch(keto_snapshot* s, const keto_expand_req* reqs, uint32_t n, int32_t global_max_depth,
                             uint32_t encoding, keto_encoded** out);
/* Same with pre-resolved roots, as keto_expand_batch_ids takes them. */
int keto_expand_encode_batch_ids(keto_snapshot* s, const uint32_t* roots, const int32_t* max_depth, uint32_t n,
                                 int32_t global_max_depth, uint32_t encoding, keto_encoded** out);
void keto_encoded_free(keto_encoded* e);                               /* NULL is fine */
uint32_t keto_encoded_count(const keto_encoded* e);                    /* n */
/* the bytes of every tree, back to back (NULL when the total is 0); *total_out = their count */
const uint8_t* keto_encoded_bytes(const keto_encoded* e, uint64_t* total_out);
const uint64_t* keto_encoded_offsets(const keto_encoded* e);           /* n + 1; tree i = bytes[off[i], off[i+1]) */
const uint8_t* keto_encoded_status(const keto_encoded* e);             /* n x KETO_EXPAND_* */

/* ---- Lists: ListRelationTuples from the snapshot (repo:keto_amd/csrc/list.hip) ----
 * keto_list_batch replaces, for a batch of queries, relationtuple.Manager.GetRelationTuples as a list:
 * ReadService.ListRelationTuples and GET /relation-tuples (internal/relationtuple/read_server.go:21-48,
 * 114-154), which end in sql.(*Persister).GetRelationTuples (internal/persistence/sql/relationtuples.go:
 * 238-277) with whereQuery (:178-198) and, for a subject, whereSubject (:151-176).  Per query the
 * result is the matching tuples in the reference's ORDER BY (:250; SQLite: subject sets before subject
 * ids), duplicates kept, rows [(page-1) * size, page * size) of them with page = max(page, 1), the
 * next page token and the count of all matches (pop's COUNT(*) behind the token):
 * next_page = page + 1 unless page >= ceil(total / size), then 0 -- so 0 when nothing matches and 0
 * past the end (:262-265).  Materialized wildcard rows (row keys with an empty field) and batch-local
 * rows are views of other rows' tuples, not tuples: they are never listed.  A stored subject set with
 * an empty field is a tuple; its `subject` names its materialized row, which keto_subject_fields
 * prints with the empty field.
 *
 * A tuple is {row id (snapshot row order), subject reference as in keto_tree_node.subject}: the caller
 * gets namespace, object and relation from keto_subject_fields(s, NULL, {row | 0x80000000}, ...) and
 * the subject from the same call.  Row ids and string ids are only ever appended by
 * keto_snapshot_apply (repo:keto_amd/csrc/delta.cpp, the commit: new strings and row keys are
 * pushed behind the existing ones, none moves), so a result stays decodable after later writes.  The
 * tuple block lives in the library's pinned pool, like a keto_encoded result's bytes, sized exactly
 * after the count pass (min(size, total - first) per query): a huge page_size allocates nothing.
 *
 * Poisoned tuples (a namespace id, or a subject set's namespace id, the config lacks: toInternal
 * fails, :43-80) have lost their subject in the snapshot.  Without a subject filter the answer is
 * still exact: KETO_LIST_NOT_FOUND iff such a tuple falls inside the page.  With a subject filter, a
 * poisoned tuple anywhere among the tuples matching the query's namespace, object and relation could
 * be a match the snapshot cannot see: the query is KETO_LIST_UNDECIDED and the caller asks the
 * reference.
 *
 * The first list call on a snapshot version builds the list index on host threads and uploads it
 * (8 B per tuple plus 8 B per row of device memory, counted in keto_snapshot_stats.device_bytes); a
 * keto_snapshot_apply leaves it stale and the next list call patches it, or rebuilds all of it
 * (keto_list_index_info, below); a keto_snapshot_delete_query patches it to the new version (below).
 * Errors: a host-only snapshot is KETO_E_HIP, any part of a partitioned upload (n_parts > 1)
 * KETO_E_INVALID; n = 0 gives count 0 and offsets {0}.  Calls take the snapshot's lock shared, as
 * keto_expand_batch does, and run one at a time per snapshot. */
#define KETO_LIST_OK 0          /* tuples, next_page and total equal the reference's */
#define KETO_LIST_NOT_FOUND 1   /* herodot.ErrNotFound: unknown query namespace or subject-set namespace
                                   (GetNamespaceByName, relationtuples.go:161,180), or a tuple OF THE PAGE
                                   fails toInternal (:43-80, :268-274); no tuples */
#define KETO_LIST_UNDECIDED 2   /* the snapshot cannot tell (above): ask the reference; no tuples */

typedef struct {
    keto_str namespace_, object, relation;  /* empty = not filtered (whereQuery :179-191) */
    uint8_t has_subject;                    /* 0: RelationQuery.Subject() == nil */
    keto_subject subject;                   /* typed, exact equality on every field (whereSubject :151-176) */
    uint32_t page_size;                     /* 0 -> the snapshot's page_size (defaultPageSize, persister.go:46,111-113) */
    uint32_t page;                          /* the decimal page token; 0 = "" = page 1 (persister.go:117-130) */
} keto_list_req;
typedef struct { uint32_t row; uint32_t subject; } keto_list_tuple;
typedef struct keto_listed keto_listed;
int keto_list_batch(keto_snapshot* s, const keto_list_req* reqs, uint32_t n, keto_listed** out);
void keto_listed_free(keto_listed*);                          /* NULL is fine */
uint32_t keto_listed_count(const keto_listed*);               /* n */
const keto_list_tuple* keto_listed_tuples(const keto_listed*, uint64_t* total_out);
const uint64_t* keto_listed_offsets(const keto_listed*);      /* n+1; query i = tuples[off[i], off[i+1]) */
const uint8_t*  keto_listed_status(const keto_listed*);       /* n x KETO_LIST_* */
const uint64_t* keto_listed_next_page(const keto_listed*);    /* 0 = "" (last page), else the token's number */
const uint64_t* keto_listed_totals(const keto_listed*);       /* matches of the whole query (pop's COUNT) */
/* of the call that made the result: index_ms = the list index (re)built first (0 when it was current),
 * scan_ms = the count, scan and emit passes on the device (HIP events) */
int keto_listed_timing(const keto_listed*, float* index_ms, float* scan_ms);
/* host only; works on device = -1 snapshots: what the scan will be asked to do.  [lo, hi) = the entries
 * of the list index (all tuples in ORDER BY order) the query is narrowed to by binary search over the
 * rows in key order (namespace: its run; namespace + object: narrower; all three: one row; lo == hi
 * when a filter names an unknown string or subject); ns / obj / rel / subject = what the scan still
 * compares per entry (obj / rel: string ids, subject: the entry word; 0xFFFFFFFF = not compared);
 * ns = the namespace id the range is the run of (INT64_MIN: no namespace filter; the scan never
 * compares it); status = KETO_LIST_OK or KETO_LIST_NOT_FOUND (unknown namespace). */
typedef struct { uint64_t lo, hi; int64_t ns; uint32_t obj, rel, subject; uint8_t status; } keto_list_plan_t;
int keto_list_plan(const keto_snapshot* s, const keto_list_req* reqs, uint32_t n, keto_list_plan_t* out);

/* ---- List response bodies encoded on the device (repo:keto_amd/csrc/list.hip, proto.hip) ----
 * keto_list_encode_batch answers the same queries as keto_list_batch with the bytes a handler sends,
 * so the caller makes no keto_subject_fields call and marshals nothing:
 *   KETO_ENC_JSON   json.Marshal(GetResponse) (internal/relationtuple/handler.go:23-29), no trailing
 *                   newline: {"relation_tuples":[T,...],"next_page_token":"<decimal or empty>"} with
 *                   T = {"namespace":..,"object":..,"relation":..,"subject_id":..} or
 *                   ..,"subject_set":{"namespace":..,"object":..,"relation":..}} --
 *                   InternalRelationTuple.MarshalJSON is ToQuery() (definitions.go:340-342,367-375), whose
 *                   RelationQuery has this field order and omitempty on the two subject fields only
 *                   (definitions.go:45-65), so empty strings print as "".  Strings are escaped as Go's
 *                   encoding/json does with HTML escaping, exactly as in keto_tree_json_all.  An empty
 *                   page is [] and never null (persistence/sql/relationtuples.go:267: make(..., len(res))).
 *   KETO_ENC_PROTO  proto.Marshal(ListRelationTuplesResponse) (read_server.go:39-45,148-151;
 *                   proto/ory/keto/acl/v1alpha1/read_service.proto:85-91, acl.proto:14-52; ToProto,
 *                   definitions.go:231-250,358-365): per tuple 0x0A len M, M = the namespace (0x0A),
 *                   object (0x12) and relation (0x1A) strings, each omitted when empty, and 0x22 len
 *                   Subject, always present, its bytes as in keto_tree_proto_all (an id is present even
 *                   when ""; a set's empty strings are omitted); then 0x12 len digits when the token is
 *                   not empty.  An OK query without tuples and without a token has no bytes: the status
 *                   tells it from a failed one.
 * Statuses, next_page, totals and the page windows are exactly keto_list_batch's on the same requests,
 * the poison rule and page_size 0 included.  A query that is not KETO_LIST_OK has an empty body (its two
 * offsets are equal).  The herodot writer's framing around the JSON is the caller's.
 * The result owns a block of the library's pinned pool and holds no reference to the snapshot: it
 * stays readable after keto_snapshot_apply and keto_snapshot_release, until it is freed.  n = 0 gives
 * count 0, offsets {0} and total 0.  Errors: an unknown encoding, out == NULL, or reqs == NULL with
 * n > 0 is KETO_E_INVALID; then as keto_list_batch: a host-only snapshot is KETO_E_HIP whatever n is, a
 * part of a partitioned upload KETO_E_INVALID.  More than 2^31 tuples in one call is KETO_E_RANGE.
 * Device memory beyond the list call's: 16 B per tuple of the pages plus the bodies.
 * KETO_LIST_ENC_LDS=0 (environment, read per call) makes every wave of the write kernel write straight
 * to global memory instead of staging its items in LDS; the bytes are the same. */
typedef struct keto_list_encoded keto_list_encoded;
int keto_list_encode_batch(keto_snapshot* s, const keto_list_req* reqs, uint32_t n,
                           uint32_t encoding /* KETO_ENC_PROTO | KETO_ENC_JSON */, keto_list_encoded** out);
void            keto_list_encoded_free(keto_list_encoded*);                 /* NULL is fine */
uint32_t        keto_list_encoded_count(const keto_list_encoded*);
const uint8_t*  keto_list_encoded_bytes(const keto_list_encoded*, uint64_t* total_out); /* NULL when total is 0 */
const uint64_t* keto_list_encoded_offsets(const keto_list_encoded*);       /* n+1; body i = bytes[off[i], off[i+1]) */
const uint8_t*  keto_list_encoded_status(const keto_list_encoded*);        /* n x KETO_LIST_* */
const uint64_t* keto_list_encoded_next_page(const keto_list_encoded*);
const uint64_t* keto_list_encoded_totals(const keto_list_encoded*);
const uint64_t* keto_list_encoded_tuples(const keto_list_encoded*);        /* n: tuples encoded into body i */
/* index_ms and scan_ms as keto_listed_timing (scan_ms ends with the emit pass: no tuple leaves the
 * device); encode_ms = sizes, scan, write and the bytes' D2H (HIP events on the list stream) */
int keto_list_encoded_timing(const keto_list_encoded*, float* index_ms, float* scan_ms, float* encode_ms);

/* The list index across writes (repo:keto_amd/csrc/list.hip).  keto_snapshot_apply leaves the index as
 * it is and only notes the ids of the rows it changed in a journal (a deduplicated set, relative to the
 * version the index describes).  The first list call after one or more writes patches the index from
 * the journal instead of rebuilding it: the host half (the rows in key order and their first entries)
 * by a merge, the device half by a splice -- a new T is written out of place from the old one and the
 * changed rows' new entries (old and new T live together until the splice is done); keys[] takes the
 * new rows' keys.  The next list call rebuilds everything, as before, when the journal holds more
 * than KETO_LIST_PATCH_MAX_ROWS distinct rows (environment, default 2^12), with KETO_LIST_PATCH=0 in
 * the environment, after a keto_snapshot_delete_query that found the index stale, or when any step of
 * the device patch fails.  keto_list_plan and a delete's host scan patch the host half alone; the device
 * half follows on the next keto_list_batch.
 *
 * keto_list_index_info reports that state; it builds nothing and works on any snapshot (all zeros
 * before the first list, plan or delete call). */
typedef struct {
    uint32_t host_built, host_current;   /* ord/first exist; and are at the snapshot's version */
    uint32_t dev_built, dev_current;     /* T/keys exist; and are at the snapshot's version */
    uint64_t host_version, dev_version;  /* valid when built */
    uint64_t entries;                    /* N of the device index (0 without one) */
    uint64_t device_bytes;
    uint32_t journal_valid;              /* 1 = the next list call can patch */
    uint32_t journal_rows;               /* distinct rows noted since dev_version (host_version without a device half) */
    uint64_t host_builds, host_patches;  /* since the handle was made */
    uint64_t dev_builds, dev_patches;    /* delete_index_patch counts as a dev_patch */
    uint64_t last_segments, last_staged_entries;   /* of the last device patch */
    float    last_host_ms, last_device_ms;         /* last build or patch: host wall; HIP events around the splice (0 for a build) */
} keto_list_index_info_t;
int keto_list_index_info(const keto_snapshot* s, keto_list_index_info_t* out);

/* ---- Delete by query: DeleteAllRelationTuples on a live snapshot (repo:keto_amd/csrc/list.hip, delta.cpp) ----
 * keto_snapshot_delete_query follows relationtuple.Manager.DeleteAllRelationTuples
 * (internal/relationtuple/definitions.go:28-34), i.e. sql.(*Persister).DeleteAllRelationTuples
 * (internal/persistence/sql/relationtuples.go:225-236): the delete behind DELETE /relation-tuples
 * (internal/relationtuple/transact_server.go:187-208) and the gRPC DeleteRelationTuples (:55-70).  Every
 * tuple matching whereQuery (:178-198) and, for a subject, whereSubject (:151-176: typed, exact on
 * every field) is removed, duplicates included; an empty query removes every tuple.  `query` is a
 * keto_list_req whose page_size and page are ignored.  A filter naming a string or subject the snapshot
 * has never seen matches nothing (KETO_OK, deleted = 0).  An unknown query namespace or subject-set
 * namespace ("" included, as for lists) fails the call with KETO_E_INVALID and changes nothing, as
 * GetNamespaceByName fails the reference's transaction (:161,180).  Materialized wildcard rows are
 * views: never matched themselves, re-materialized when a row their query returns lost a tuple; a
 * stored subject set with an empty field is a tuple, matched by its subject word as in a list.
 *
 * Every successful call bumps the version by 1, like keto_snapshot_apply, also when nothing matched:
 * replicas and parts given the same calls stay at equal versions.  A shared-rows part and a host-only
 * snapshot take the call; a migrating part takes none (KETO_E_INVALID).  Locking is
 * keto_snapshot_apply's: the scan and the staging run under the shared lock (batches keep running), the
 * commit under the exclusive one.
 *
 * KETO_E_REBUILD (snapshot unchanged: same version, same answers; the caller rebuilds): a matched tuple
 * is a poisoned one; the query has a subject and a poisoned tuple lies among the tuples matching its
 * namespace / object / relation part (the list call's KETO_LIST_UNDECIDED rule); a touched row, or a
 * wildcard row matching one, is poisoned; or more than KETO_DELETE_QUERY_MAX_ROWS rows (environment,
 * default 2^20) are touched -- every touched row is re-imaged on the device, so past some size a rebuild
 * is the cheaper answer.
 *
 * Who finds the rows: the host (candidate rows by the resolver's binary searches, scanned on host
 * threads) on a host-only snapshot, a part, when the device list index is not current at this version
 * -- a delete never builds it -- or when namespace, object and relation are all given (one row); the
 * device (a count / scan / emit pass over the list index, as in keto_list_batch) otherwise.  A device
 * list index that was current is patched out of place to the new version (8 B less per deleted tuple)
 * instead of being rebuilt by the next list call; if the patch fails the index is dropped and the next
 * list call rebuilds it -- the delete has happened either way. */
#define KETO_DELETE_PATH_HOST 0
#define KETO_DELETE_PATH_DEVICE 1
typedef struct {
    uint64_t deleted;       /* tuples removed (SQL: rows affected) */
    uint64_t rows_touched;  /* distinct (namespace_id, object, relation) rows that lost a tuple */
    uint64_t version;       /* the snapshot's version after the call */
    uint32_t path;          /* KETO_DELETE_PATH_HOST | KETO_DELETE_PATH_DEVICE: who found the rows */
    uint32_t index_kept;    /* 1 = the device list index was patched and is current at `version` */
    float    scan_ms;       /* finding the rows (host wall time, or HIP events on the list stream) */
    float    apply_ms;      /* staging + commit + device_apply, and the index patch */
} keto_delete_info;
int keto_snapshot_delete_query(keto_snapshot* s, const keto_list_req* query, keto_delete_info* out /* may be NULL */);

/* ---- Reverse lookup: the objects a subject has a relation on (repo:keto_amd/csrc/list.hip) ----
 * keto_lookup_objects_batch answers, per query, "which objects o of `namespace_` does `subject` have
 * `relation` on": a question the reference has no call for -- there it costs one
 * check.(*Engine).SubjectIsAllowed (internal/check/engine.go:116-123) per candidate object.  Query i
 * answers with the row ids of the tuple rows (namespace_, o, relation) whose check against `subject`,
 * at the same request and global max-depth, is allowed: for every non-empty o that is keto_check_batch
 * on namespace_:o#relation@subject returning allowed with KETO_CHECK_OK; a tuple row whose object is
 * the empty string is checked as that one row, by row id (a named request with an empty object would
 * be a wildcard query over every object instead).  Rows come in key order, i.e. in ascending byte order of o; the page is rows
 * [(page-1) * size, page * size) of them with page = max(page, 1), next_page and the total follow the
 * list rule (above), the total being the allowed objects of the whole query.  The caller decodes a row
 * with keto_subject_fields(s, NULL, {row | 0x80000000}, ...), exactly as for list tuples; row ids stay
 * decodable after later writes.
 *
 * Nothing is traversed backwards: the candidates of a query are the distinct tuple rows of its
 * namespace and relation, taken from the list index in key order (the HEAD passes that
 * keto_snapshot_delete_query uses), and every candidate is checked forwards by the check kernels, on
 * the device, as a keto_check_batch_rows_device request.  An object with no tuple at that relation
 * can never be allowed (the check reads the top-level row's tuples, engine.go:82-114), so the tuple
 * rows are the complete candidate set, and the set returned is exactly the set this engine's check
 * allows.  Candidates, requests and decisions stay in device memory; the page of allowed row ids is
 * all that comes back.  A subject the snapshot does not know is not an error: every check is false
 * (KETO_LOOKUP_OK, total 0).  A poisoned top-level row is simply a candidate: the check truncates it
 * at its first poisoned page, as it does for keto_check_batch.
 *
 * namespace_ and relation are both required and taken literally, as a check request's are.  An empty
 * namespace_ or relation, or a subject set with an empty field, would be a wildcard check, which needs
 * batch-local rows: KETO_LOOKUP_UNSUPPORTED for that query (ask keto_check_batch); the other queries
 * of the batch are answered as usual.
 *
 * Errors, as for lists: a host-only snapshot is KETO_E_HIP (whatever n is), any part of a partitioned
 * upload (n_parts > 1) KETO_E_INVALID; n = 0 gives count 0 and offsets {0}.  More than
 * KETO_LOOKUP_MAX_CANDIDATES candidates (environment, default 2^28) over the queries of one call fail
 * the call with KETO_E_INVALID before any check runs.  Candidates are checked in chunks of
 * KETO_LOOKUP_CHUNK (environment, default 2^22, at least 64).  The call holds the snapshot's lock
 * shared from start to end, so every decision belongs to one version, and runs one at a time per
 * snapshot with the list calls, whose index and stream it shares (the first call on a version builds
 * or patches the list index exactly as keto_list_batch does).  Device memory beyond the list index:
 * 5 B per candidate (row id and decision), 16 B per candidate of a chunk (its request; the check
 * keeps a translated copy of as many), 4 B per emitted row; the candidate, decision and request
 * buffers are kept for the next call up to 256 MB each and freed at the end of a call past that (they
 * are not counted in keto_snapshot_stats.device_bytes).  The result owns a block of the pinned
 * pool sized exactly after the totals (a huge page_size allocates nothing) and holds no reference to
 * the snapshot: it stays readable after keto_snapshot_apply and keto_snapshot_release, until
 * keto_looked_free. */
#define KETO_LOOKUP_OK 0                 /* rows, next_page, total equal per-object SubjectIsAllowed */
#define KETO_LOOKUP_UNKNOWN_NAMESPACE 1  /* query namespace unknown: every check is false; no rows, total 0 */
#define KETO_LOOKUP_UNDECIDED 2          /* >= 1 candidate's check was KETO_UNDECIDED: no rows, total 0; `undecided` says how many */
#define KETO_LOOKUP_UNSUPPORTED 3        /* empty namespace or relation, or a subject set with an empty field
                                            (wildcard checks need batch-local rows): ask keto_check_batch */
typedef struct {
    keto_str namespace_, relation;   /* both required, taken literally as a check request's are */
    keto_subject subject;
    int32_t  max_depth;              /* <= 0 or > global -> global, as keto_check_req */
    uint32_t page_size;              /* 0 -> the snapshot's page_size */
    uint32_t page;                   /* 0 = page 1 */
} keto_lookup_req;
typedef struct keto_looked keto_looked;
int keto_lookup_objects_batch(keto_snapshot* s, const keto_lookup_req* reqs, uint32_t n,
                              int32_t global_max_depth, keto_looked** out);
void keto_looked_free(keto_looked*);                       /* NULL is fine */
uint32_t        keto_looked_count(const keto_looked*);     /* n */
const uint32_t* keto_looked_rows(const keto_looked*, uint64_t* total_out);  /* row ids (NULL when there are none) */
const uint64_t* keto_looked_offsets(const keto_looked*);    /* n+1; query i = rows[off[i], off[i+1]) */
const uint8_t*  keto_looked_status(const keto_looked*);     /* n x KETO_LOOKUP_* */
const uint64_t* keto_looked_next_page(const keto_looked*);  /* the list rule: 0 on the last page, when nothing matches, or past the end */
const uint64_t* keto_looked_totals(const keto_looked*);     /* allowed objects of the whole query */
const uint64_t* keto_looked_candidates(const keto_looked*); /* rows checked for the query */
const uint64_t* keto_looked_undecided(const keto_looked*);  /* of them: checks that ended KETO_UNDECIDED */
/* of the call that made the result: index_ms = the list index (re)built first (0 when it was current);
 * HIP events on the list stream: candidates_ms = the HEAD count, scan and emit, check_ms = the
 * chunks' requests and checks, emit_ms = the count, scan and emit of the allowed rows and their copy */
int keto_looked_timing(const keto_looked*, float* index_ms, float* candidates_ms, float* check_ms, float* emit_ms);

/* ---- Subjects of an object: Expand flattened on the device (repo:keto_amd/csrc/subjects.hip) ----
 * keto_subjects_batch answers, per query, "which subjects have `relation` on `namespace_`:`object`".
 * Keto v0.8.1 has no call for it: a caller expands the subject set and flattens the tree.  This call
 * does exactly that, on the device.  Let T be the tree keto_expand_batch returns for the subject set
 * namespace_:object#relation at the request's max_depth, clamped as BuildTree clamps it
 * (internal/expand/engine.go:35-37).  Query i answers with the DISTINCT SubjectID LEAVES OF T, each as
 * its string id (the keto_tree_node.subject word, bit 31 clear; decode with
 * keto_subject_fields(s, NULL, ...)), in ASCENDING STRING-ID ORDER; the page is ids
 * [(page-1) * size, page * size) of them with page = max(page, 1), page_size 0 = the snapshot's page
 * size; next_page and the total follow the list rule (above), the total being the number of distinct
 * SubjectID leaves.
 *
 * The order is the string id's, not the bytes'.  String ids are in byte order for every string present
 * when the snapshot was built; strings added by keto_snapshot_apply are appended and no id ever moves
 * (see the list section).  So a subject first written after the build sorts behind every older one
 * whatever its bytes, and a page token stays meaningful across writes: the ids before a page only
 * change when a subject of the set itself comes or goes.  Byte order would need a rank table over all
 * strings per version.
 *
 * This is Expand's answer with Expand's quirks -- one visited map per tree, the depth cut at
 * restDepth <= 1, nil children turned into leaves -- NOT "every subject for which a check is allowed".
 * The two agree when the depth is ample and no subject set is visited twice on different paths; they
 * can differ otherwise.  The check-semantics variant is keto_allowed_subjects_batch (below).  Per query the call reports what tells
 * the caller so: `leaves` = the SubjectID leaf nodes of T before deduplication, `set_leaves` = the leaf
 * nodes of T whose subject is a subject set (depth-cut, revisited or empty sets; a node count, not a
 * distinct count).  set_leaves != 0: the list may be cut short by the depth.  Subject-set leaves are
 * not returned as subjects (they may name batch-local wildcard rows only an arena can decode): a caller
 * who needs them asks keto_expand_batch.
 *
 * A query with an empty field is a wildcard root and goes through the batch's overlay exactly as in
 * keto_expand_batch; its id leaves are ordinary string ids.  KETO_SUBJECTS_NOT_FOUND is
 * KETO_EXPAND_NOT_FOUND (unknown namespace), KETO_SUBJECTS_UNDECIDED is KETO_EXPAND_UNDECIDED (no ids,
 * total 0: ask the reference); a nil tree is KETO_SUBJECTS_OK with total 0 and set_leaves 0.
 *
 * On the device: the expand leaves its node arena in the snapshot's buffers (as for
 * keto_expand_encode_batch); a 64-bit scan over the id-leaf flags and a compaction give each tree its
 * segment of leaf words; a segment is sorted and made distinct by one of three kernels chosen by its
 * length L: L <= 64 a wave (bitonic network over the lanes), L <= KETO_SUBJECTS_LDS (environment,
 * default 2048; a power of two in [128, 8192], anything else fails the call with KETO_E_INVALID) a
 * block sorting in LDS, longer ones one radix sort over 64-bit (segment, word) keys and a streaming
 * unique; one kernel copies the windows, one DMA brings the page back.  Device memory, derived, not
 * measured: 8 B of scan and 4 B of leaf words per NODE of the arena (the leaf buffer is sized for the
 * bound, every node; 4 B per id leaf are used), 8 B twice per id leaf of the radix-sorted class (the
 * sort is out of place), 64 B per query (segment start, three counts, class lists, window), 4 B per
 * emitted id; each buffer is kept for the next call up to 256 MB and freed at the end of the call past
 * that (not counted in keto_snapshot_stats.device_bytes).  More than 2^31 - 1 leaves in the
 * radix-sorted class fail the call with KETO_E_RANGE.
 *
 * The result owns a block of the pinned pool sized exactly after the totals (a huge page_size
 * allocates nothing) and holds no reference to the snapshot: it stays readable after
 * keto_snapshot_apply and keto_snapshot_release, until keto_subjects_free.  Errors, as for
 * keto_expand_encode_batch: NULL arguments are KETO_E_INVALID, checked first; a host-only snapshot is
 * KETO_E_HIP whatever n is; a migrating part (KETO_PART_MIGRATE, n_parts > 1) and a root owned by
 * another shared-rows part are KETO_E_INVALID; n = 0 gives count 0 and offsets {0}.  The call takes
 * the snapshot's lock shared from the expand to the page, the device state's mutex for the expand and
 * the passes over its arena, and runs one flatten at a time per snapshot. */
#define KETO_SUBJECTS_OK 0          /* ids, next_page, total = the distinct SubjectID leaves of the expand tree */
#define KETO_SUBJECTS_NOT_FOUND 1   /* KETO_EXPAND_NOT_FOUND: unknown namespace; no ids, total 0 */
#define KETO_SUBJECTS_UNDECIDED 2   /* KETO_EXPAND_UNDECIDED: the tree exceeded the engine's limits; no ids, total 0 */
typedef struct {
    keto_str namespace_, object, relation;  /* the subject set to expand; an empty field = a wildcard root */
    int32_t  max_depth;                     /* <= 0 or > global -> global, as keto_expand_req */
    uint32_t page_size;                     /* 0 -> the snapshot's page_size */
    uint32_t page;                          /* 0 = page 1 */
} keto_subjects_req;
typedef struct keto_subjects keto_subjects;
int keto_subjects_batch(keto_snapshot* s, const keto_subjects_req* reqs, uint32_t n, int32_t global_max_depth,
                        keto_subjects** out);
/* Same with pre-resolved roots, as keto_expand_batch_ids takes them; page_size and page hold n entries
 * each.  Every root must have bit 31 set (a subject set's row): one without fails the call with
 * KETO_E_INVALID before *out is touched. */
int keto_subjects_batch_ids(keto_snapshot* s, const uint32_t* roots, const int32_t* max_depth,
                            const uint32_t* page_size, const uint32_t* page, uint32_t n, int32_t global_max_depth,
                            keto_subjects** out);
void keto_subjects_free(keto_subjects*);                        /* NULL is fine */
uint32_t        keto_subjects_count(const keto_subjects*);      /* n */
const uint32_t* keto_subjects_ids(const keto_subjects*, uint64_t* total_out);  /* string ids (NULL when there are none) */
const uint64_t* keto_subjects_offsets(const keto_subjects*);    /* n+1; query i = ids[off[i], off[i+1]) */
const uint8_t*  keto_subjects_status(const keto_subjects*);     /* n x KETO_SUBJECTS_* */
const uint64_t* keto_subjects_next_page(const keto_subjects*);  /* the list rule: 0 on the last page, when there is nothing, or past the end */
const uint64_t* keto_subjects_totals(const keto_subjects*);     /* distinct SubjectID leaves of the whole tree */
const uint64_t* keto_subjects_leaves(const keto_subjects*);     /* SubjectID leaf nodes before deduplication */
const uint64_t* keto_subjects_set_leaves(const keto_subjects*); /* leaf nodes whose subject is a subject set */
/* of the call that made the result: expand_ms = the expand half (host wall time, as a caller pays it),
 * flatten_ms = everything after it on the flatten's stream (HIP events) */
int keto_subjects_timing(const keto_subjects*, float* expand_ms, float* flatten_ms);
/* five HIP-event times in ms: the scan and compaction, the wave class, the block class, the radix-sorted
 * class, the counts' copy + windows + emit + the page's DMA (NULL for a NULL result) */
const float* keto_subjects_stages(const keto_subjects*);

/* ---- Subjects a check allows on an object (repo:keto_amd/csrc/allowed.hip) ----
 * keto_allowed_subjects_batch answers, per query {namespace_, object, relation, max_depth, page_size,
 * page}, "who may touch this object" with CHECK semantics: the SubjectIDs S for which keto_check_batch
 * on namespace_:object#relation@S, at the same request and global max-depth, returns allowed with
 * KETO_CHECK_OK.  It is the mirror of keto_lookup_objects_batch and the check-semantics counterpart of
 * keto_subjects_batch (which flattens Expand's tree and carries Expand's quirks instead): the ids come
 * back as string ids (decode with keto_subject_fields(s, NULL, ...)) in ascending string-id order, for
 * the reason given in the keto_subjects_batch section (a page token stays meaningful across writes; a
 * subject first written after the build sorts last); the page is ids [(page-1) * size, page * size)
 * with page = max(page, 1), page_size 0 = the snapshot's page size; next_page and the total follow the
 * list rule, the total being the number of allowed subject ids of the whole query.  Subject-set
 * subjects are NOT returned (the question "which subject sets does a check allow" has no finite
 * candidate set of stored rows alone; ask keto_check_batch), and there is no partitioned variant.
 *
 * Nothing is traversed with the check's quirks twice: a check at clamped depth d says yes only when a
 * row it enters holds the requested id, and it enters only rows within d - 1 subject-set hops of the
 * request's row (internal/check/engine.go:54, 88-91).  So the id edges of all rows within d - 1 hops of
 * the row (namespace_, object, relation), over the stored effective subject-set edges, hold every id
 * that can be allowed: a superset, gathered by a hop-bounded, level-synchronous BFS over the device
 * arena for all queries at once (frontier keys deduplicated in a device hash table, so cycles and shared
 * substructure cost each row once per query).  The distinct candidates are then checked forwards by the
 * check kernels, each exactly as a keto_check_batch_rows_device request, and the allowed ones compacted
 * in order: the set returned is exactly the set this engine's check allows, visited-map quirks
 * included.  Per query, `candidates` = the distinct ids that were checked and `undecided` = of them, the
 * checks that ended KETO_UNDECIDED; a query with one or more of those is KETO_ALLOWED_UNDECIDED and
 * returns nothing (ask the reference).  An object or relation string the snapshot has never seen, or a
 * key with no row, is KETO_ALLOWED_OK with total 0 and candidates 0.  An empty namespace, object or
 * relation would be a wildcard query, which needs a batch-local row: KETO_ALLOWED_UNSUPPORTED for that
 * query, the other queries of the batch being answered as usual.
 *
 * Errors, as for keto_lookup_objects_batch: NULL arguments are KETO_E_INVALID, checked first; a
 * host-only snapshot is KETO_E_HIP whatever n is; any part of a partitioned upload (n_parts > 1) is
 * KETO_E_INVALID; n = 0 gives count 0 and offsets {0}.  More than KETO_ALLOWED_MAX_CANDIDATES
 * (environment, default 2^28) id edges gathered over the queries of one call fail the call with
 * KETO_E_INVALID before any check runs; the test is made on an upper bound taken from the rows' headers
 * (a row walked edge by edge counts every word, its subject sets included, and poisoned edges count), so
 * a call can be refused with somewhat fewer id edges than the limit, never accepted with more.  Candidates are checked in chunks of KETO_ALLOWED_CHUNK
 * (environment, default 2^22, at least 64); KETO_ALLOWED_VISITED_SLOTS (environment) sets the initial
 * size of the BFS's visited table (and the number of keys it is sized for ahead of a level without being
 * asked, by default 2^16 or four times the keys visited so far); a level that would fill it past half
 * reports that, the table is sized for the level's set edges and the level runs again, at most once.  The call
 * holds the snapshot's lock shared from start to end, so candidates, checks and page belong to one
 * version, and runs one at a time per snapshot on a workspace and stream of its own.  Device memory,
 * derived, not measured: 8 B per visited (query, row) key and 8 B per slot of the visited table (at
 * least twice the keys; after a level ran again, twice that level's set edges), 12 B twice per row of a
 * level (tile count and scan, of two levels), 8 B twice per gathered id edge
 * (the sort is out of place; the second buffer holds the ranks later), 5 B per distinct candidate (id and
 * decision), 16 B per candidate of a chunk (its request; the check keeps a translated copy of as many),
 * 4 B per emitted id; each buffer is kept for the next call up to 256 MB and freed at the end of a call
 * past that (not counted in keto_snapshot_stats.device_bytes).  The result owns a block of the pinned
 * pool sized exactly after the totals (a huge page_size allocates nothing) and holds no reference to
 * the snapshot: it stays readable after keto_snapshot_apply and keto_snapshot_release, until
 * keto_allowed_free. */
#define KETO_ALLOWED_OK 0                 /* ids, next_page, total equal per-subject SubjectIsAllowed */
#define KETO_ALLOWED_UNKNOWN_NAMESPACE 1  /* query namespace unknown: every check is false; no ids, total 0 */
#define KETO_ALLOWED_UNDECIDED 2          /* >= 1 candidate's check was KETO_UNDECIDED: no ids, total 0; `undecided` says how many */
#define KETO_ALLOWED_UNSUPPORTED 3        /* empty namespace, object or relation (a wildcard query needs a
                                             batch-local row): ask keto_check_batch */
typedef struct {
    keto_str namespace_, object, relation;  /* all required, taken literally as a check request's are */
    int32_t  max_depth;                     /* <= 0 or > global -> global, as keto_check_req */
    uint32_t page_size;                     /* 0 -> the snapshot's page_size */
    uint32_t page;                          /* 0 = page 1 */
} keto_allowed_req;
typedef struct keto_allowed keto_allowed;
int keto_allowed_subjects_batch(keto_snapshot* s, const keto_allowed_req* reqs, uint32_t n,
                                int32_t global_max_depth, keto_allowed** out);
void keto_allowed_free(keto_allowed*);                        /* NULL is fine */
uint32_t        keto_allowed_count(const keto_allowed*);      /* n */
const uint32_t* keto_allowed_ids(const keto_allowed*, uint64_t* total_out);  /* string ids (NULL when there are none) */
const uint64_t* keto_allowed_offsets(const keto_allowed*);    /* n+1; query i = ids[off[i], off[i+1]) */
const uint8_t*  keto_allowed_status(const keto_allowed*);     /* n x KETO_ALLOWED_* */
const uint64_t* keto_allowed_next_page(const keto_allowed*);  /* the list rule: 0 on the last page, when there is nothing, or past the end */
const uint64_t* keto_allowed_totals(const keto_allowed*);     /* allowed subject ids of the whole query */
const uint64_t* keto_allowed_candidates(const keto_allowed*); /* distinct ids checked for the query */
const uint64_t* keto_allowed_undecided(const keto_allowed*);  /* of them: checks that ended KETO_UNDECIDED */
/* of the call that made the result, HIP events on the call's stream: bfs_ms = the seeds and the levels,
 * dedupe_ms = sort, unique and split, check_ms = the chunks' requests and checks, emit_ms = the rank
 * scan, the totals, the page and its copy */
int keto_allowed_timing(const keto_allowed*, float* bfs_ms, float* dedupe_ms, float* check_ms, float* emit_ms);
/* the BFS of the call that made the result (any pointer may be NULL): the (query, row) keys it visited, the
 * slots of the visited table at the end, the rows it met that a write had moved (forwarded headers; a level
 * counted twice counts them twice), the levels it ran, how often the table was enlarged ahead of a level,
 * and how often a level's emit ran again because the table proved too small for it */
int keto_allowed_bfs(const keto_allowed*, uint64_t* visited, uint64_t* slots, uint64_t* forwards, uint32_t* levels,
                     uint32_t* regrows, uint32_t* reruns);

/* The fields of subject references as keto_tree_node.subject holds them, for building expand.Tree
 * values (internal/expand/tree.go:26-30: relationtuple.SubjectID / SubjectSet,
 * internal/relationtuple/definitions.go:40-42,102-117) straight from the node arena without a text
 * codec.  a: the arena the references come from (its batch-local wildcard roots and subject ids the
 * snapshot does not know), or NULL.  Reference i: lens_out[3i..3i+2] = (id length, 0, 0) for a subject
 * id, (namespace, object, relation lengths) for a subject set; the strings follow one another in buf
 * in that order.  buf is written only if cap >= the total byte count, which is returned (call with
 * buf = NULL to size it; the count of a reference never changes, so a size-then-fill pair agrees
 * even across keto_snapshot_apply). */
int64_t keto_subject_fields(const keto_snapshot* s, const keto_tree_arena* a, const uint32_t* subjects, uint64_t n,
                            char* buf, uint64_t cap, uint32_t* lens_out);

/* String of a subject reference used in keto_tree_node.subject (Subject.String(), definitions.go:163-169). */
int64_t keto_subject_string(const keto_snapshot* s, uint32_t subject, char* buf, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* KETO_MI355X_H */
