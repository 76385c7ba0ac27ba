//go:build keto_gpu
// +build keto_gpu

package sql

import (
	"context"
	"strconv"

	"github.com/ory/x/sqlcon"

	"github.com/ory/keto/internal/gpu"
	"github.com/ory/keto/internal/relationtuple"
	"github.com/ory/keto/internal/x"
)

// snapshotChunk is the page size of the full scan (keyset pagination, so the scan stays linear).
const snapshotChunk = 1 << 20

// SnapshotRows reads this network's rows of keto_relation_tuples in commit order, the one full
// scan the GPU snapshot is built from instead of the per-node paged queries of GetRelationTuples
// (relationtuples.go:238-277).  Ties of the reference ORDER BY (relationtuples.go:250) end in
// commit_time, so commit order is all the builder needs; it sorts the rest itself.  Rows whose
// namespace id is not configured are kept: they are the poisoned pages the engines must reproduce.
func (p *Persister) SnapshotRows(ctx context.Context) ([]gpu.Row, error) {
	var out []gpu.Row
	var last *RelationTuple
	for {
		q := p.QueryWithNetwork(ctx).Order("commit_time, shard_id").Limit(snapshotChunk)
		if last != nil {
			q = q.Where("(commit_time > ?) OR (commit_time = ? AND shard_id > ?)", last.CommitTime, last.CommitTime, last.ID)
		}
		var res relationTuples
		if err := q.All(&res); err != nil {
			return nil, sqlcon.HandleError(err)
		}
		for _, r := range res {
			row := gpu.Row{NamespaceID: r.NamespaceID, Object: r.Object, Relation: r.Relation}
			if r.SubjectID.Valid {
				id := r.SubjectID.String
				row.SubjectID = &id
			} else {
				row.SetNamespaceID = r.SubjectSetNamespaceID.Int32
				row.SetObject = r.SubjectSetObject.String
				row.SetRelation = r.SubjectSetRelation.String
			}
			out = append(out, row)
		}
		if len(res) < snapshotChunk {
			return out, nil
		}
		last = res[len(res)-1]
	}
}

// GetRelationTuplesFromSnapshot is GetRelationTuples (relationtuples.go:238-277) as a list -- what
// ReadService.ListRelationTuples and GET /relation-tuples call (internal/relationtuple/
// read_server.go:21-48,114-154) -- answered from the GPU snapshot (keto_list_batch): the same tuples
// in the same ORDER BY, the same next page token.  SQL answers instead, through the embedded method,
// when the snapshot is stale or partitioned, when it cannot decide the query (gpu.ListUndecided: a
// subject filter over tuples of an unconfigured namespace), when the reference would return an error
// (gpu.ListNotFound: SQL returns the very herodot error), and for a malformed, zero or negative token
// or size, which parsePageToken (persister.go:117-130) and pop treat in ways not restated here.
//
// list is the GPU side, the registry's snapshot state (gpuState.ListTuples,
// internal/driver/registry_gpu.go): its ok is false when no snapshot can answer right now -- it is
// stale (a rebuild is under way) or partitioned.
func (p *Persister) GetRelationTuplesFromSnapshot(ctx context.Context,
	list func(qs []gpu.ListQuery) (res []gpu.ListResult, ok bool, err error), query *relationtuple.RelationQuery,
	options ...x.PaginationOptionSetter) ([]*relationtuple.InternalRelationTuple, string, error) {
	sqlAnswer := func() ([]*relationtuple.InternalRelationTuple, string, error) {
		return p.GetRelationTuples(ctx, query, options...)
	}
	if list == nil || query == nil {
		return sqlAnswer()
	}
	opts := x.GetPaginationOptions(options...)
	if opts.Size < 0 || int64(opts.Size) > 1<<31-1 {
		return sqlAnswer()
	}
	size := opts.Size
	if size == 0 {
		size = defaultPageSize
	}
	page := uint64(0) // the empty token: page 1
	if opts.Token != "" {
		v, err := strconv.ParseUint(opts.Token, 10, 32)
		if err != nil || v == 0 {
			return sqlAnswer()
		}
		page = v
	}
	res, ok, err := list([]gpu.ListQuery{{Namespace: query.Namespace, Object: query.Object, Relation: query.Relation,
		Subject: query.Subject(), PageSize: uint32(size), Page: uint32(page)}})
	if err != nil || !ok || len(res) != 1 || res[0].Status != gpu.ListOK {
		return sqlAnswer()
	}
	next := ""
	if res[0].NextPage != 0 {
		next = strconv.FormatUint(res[0].NextPage, 10)
	}
	return res[0].Tuples, next, nil
}
