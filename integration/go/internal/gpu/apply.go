//go:build keto_gpu
// +build keto_gpu

package gpu

/*
#include "keto_mi355x.h"
*/
import "C"

import (
	"context"
	"errors"

	"github.com/ory/keto/internal/namespace"
	"github.com/ory/keto/internal/relationtuple"
)

// ErrRebuild: the write touches a poisoned row (a tuple of an unconfigured namespace) or a wildcard
// row that matches one.  The snapshot is unchanged; build a new one from the table
// (keto_snapshot_apply, KETO_E_REBUILD).  New Subject.String() collisions, wildcard subject sets and
// writes to a shared-rows part of an edge-partitioned snapshot are applied in place.
var ErrRebuild = errors.New("keto_mi355x: write needs a snapshot rebuild")

// Apply patches the snapshot with one transaction of TransactRelationTuples
// (internal/persistence/sql/relationtuples.go:279-297): inserts land after the equal tuples already
// in their row (commit order), deletes remove every equal tuple.  The library takes the snapshot's
// lock exclusively, so running batches finish on the old version first.  Version is the snaptoken
// the reference leaves "not yet implemented" (internal/check/handler.go:182).
func (s *Snapshot) Apply(inserts, deletes []Row) error {
	var m cmem
	defer m.free()
	m.strings(rowsLen(inserts) + rowsLen(deletes))
	ci := m.tuples(inserts)
	cd := m.tuples(deletes)
	var v C.uint64_t
	rc := C.keto_snapshot_apply(s.h, ci, C.uint64_t(len(inserts)), cd, C.uint64_t(len(deletes)), &v)
	if rc == C.KETO_E_REBUILD {
		return ErrRebuild
	}
	if rc != C.KETO_OK {
		return lastErr(rc)
	}
	s.Version = uint64(v)
	return nil
}

// DeleteInfo is what a delete by query did (keto_delete_info).
type DeleteInfo struct {
	Deleted     uint64 // tuples removed: the SQL delete's rows affected
	RowsTouched uint64 // distinct (namespace, object, relation) rows that lost a tuple
	Version     uint64
	OnDevice    bool // the device found the rows (the list index was current), not the host
	IndexKept   bool // the device list index was patched and is current at Version
	ScanMs      float32
	ApplyMs     float32
}

// DeleteQuery follows sql.(*Persister).DeleteAllRelationTuples
// (internal/persistence/sql/relationtuples.go:225-236): every tuple matching q's whereQuery /
// whereSubject (:178-198, :151-176) leaves the snapshot (keto_snapshot_delete_query); q's PageSize
// and Page are ignored.  ErrRebuild as for Apply (a poisoned tuple is or may be among the matches, or
// more rows are touched than KETO_DELETE_QUERY_MAX_ROWS): the snapshot is unchanged.  An unknown
// namespace is an error and changes nothing -- the SQL delete has failed the same way before the
// persister gets here.  The version moves by one also when nothing matched.
func (s *Snapshot) DeleteQuery(q ListQuery) (DeleteInfo, error) {
	var m cmem
	defer m.free()
	m.strings(len(q.Namespace) + len(q.Object) + len(q.Relation) + subjectLen(q.Subject))
	cr := (*C.keto_list_req)(m.alloc(int(C.sizeof_keto_list_req)))
	*cr = C.keto_list_req{namespace_: m.s(q.Namespace), object: m.s(q.Object), relation: m.s(q.Relation)}
	if q.Subject != nil {
		cr.has_subject = 1
		cr.subject = m.subject(q.Subject)
	}
	var info C.keto_delete_info
	rc := C.keto_snapshot_delete_query(s.h, cr, &info)
	if rc == C.KETO_E_REBUILD {
		return DeleteInfo{}, ErrRebuild
	}
	if rc != C.KETO_OK {
		return DeleteInfo{}, lastErr(rc)
	}
	s.Version = uint64(info.version)
	return DeleteInfo{Deleted: uint64(info.deleted), RowsTouched: uint64(info.rows_touched), Version: uint64(info.version),
		OnDevice: info.path == C.KETO_DELETE_PATH_DEVICE, IndexKept: info.index_kept != 0,
		ScanMs: float32(info.scan_ms), ApplyMs: float32(info.apply_ms)}, nil
}

// RowsOf maps the tuples of one TransactRelationTuples call to table rows with the namespace name ->
// id lookups RelationTuple.FromInternal / insertSubject make before the SQL insert
// (internal/persistence/sql/relationtuples.go:82-130).  The persister calls Apply with them after
// its transaction commits, so the snapshot follows the table one transaction at a time.
func RowsOf(ctx context.Context, nm namespace.Manager, ts []*relationtuple.InternalRelationTuple) ([]Row, error) {
	rows := make([]Row, 0, len(ts))
	for _, t := range ts {
		n, err := nm.GetNamespaceByName(ctx, t.Namespace)
		if err != nil {
			return nil, err
		}
		r := Row{NamespaceID: n.ID, Object: t.Object, Relation: t.Relation}
		switch s := t.Subject.(type) {
		case *relationtuple.SubjectID:
			id := s.ID
			r.SubjectID = &id
		case *relationtuple.SubjectSet:
			sn, err := nm.GetNamespaceByName(ctx, s.Namespace)
			if err != nil {
				return nil, err
			}
			r.SetNamespaceID, r.SetObject, r.SetRelation = sn.ID, s.Object, s.Relation
		}
		rows = append(rows, r)
	}
	return rows, nil
}
