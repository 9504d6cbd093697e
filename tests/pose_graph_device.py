"""Helpers of the GPU pose-graph tests: model graphs (pose_graph_model.Graph) loaded into streams of a device PoseGraph."""
import numpy as np
import torch

import pose_graph_model as pgm


def load(pg, graphs, streams=None):
    """Loads the model graphs into the streams (default 0, 1, ..) of pg through append / add_loop / add_absolute."""
    streams = list(range(len(graphs))) if streams is None else list(streams)
    dev, S = pg.device, pg.streams
    longest = max(g.n for g in graphs)
    for k in range(1, longest):
        rel = torch.eye(4, dtype=torch.float64).repeat(S, 1, 1)
        act = torch.zeros(S, dtype=torch.int32)
        for g, s in zip(graphs, streams):
            if k < g.n:
                rel[s] = torch.from_numpy(g.Z[k])
                act[s] = 1
        pg.append(rel.to(dev), active=act.to(dev))
    for g, s in zip(graphs, streams):
        for i, j, Z, Om in g.loops:
            pg.add_loop(s, i, j, Z, Om)
        for i, G, Om in g.absolutes:
            pg.add_absolute(s, i, G, Om)


def make(graphs, S=None, streams=None, **kw):
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    g0 = graphs[0]
    pg = PoseGraph(S or len(graphs), max_poses=g0.N, max_loops=g0.ML, max_absolute=g0.MA, fix_first=g0.fix_first, **kw)
    load(pg, graphs, streams)
    return pg


def snapshot(pg):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in pg.bufs.items()}
