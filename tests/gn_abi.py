"""The global Gauss-Newton entry points of libmslam_hip (include/mslam_hip.h) on one input set of tests/gn_ref.py, called
through mslam_hip.lib() directly: the closed loops, the opened-up loop and the loop state.  Helper of
tests/test_gn_blocks_gpu.py and tests/test_gn_loop_gpu.py; every call owns its arguments, nothing is cached."""
import numpy as np
import torch

KIND = {"rays": 0, "calib": 1, "points": 2}
DONE, ITERS, CHOL_FAIL, LAST_NORM = range(4)


class Gn:
    def __init__(self, c, device, local_edges=None):
        import mslam_hip as m

        self.m, self.L, self.c, self.device = m, m.lib(), c, device
        g = c["g"]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.Twc0, self.Xs, self.Cs, self.K = t(g["Twc"]), t(g["Xs"]), t(g["Cs"]), t(g["K"])
        self.ii, self.jj, self.idx, self.Q = t(g["ii"]), t(g["jj"]), t(g["idx_ii2jj"]), t(g["Q"])
        self.vm = t(np.asarray(g["valid_match"]).astype(np.uint8))
        self.P, self.E, self.HW = c["P"], c["E"], c["HW"]
        self.dims = (self.P, self.HW, self.E)
        nbytes = self.L.mslam_gn_workspace_bytes(self.P, self.E, self.HW, self.E if local_edges is None else local_edges)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.wsargs = (m.ptr(self.ws), self.ws.numel(), m.stream_ptr())

    def buffers(self, fill=0.0):
        """Caller-side Hs f32[4,E,7,7], gs f32[2,E,7]."""
        return (torch.full((4, self.E, 7, 7), fill, dtype=torch.float32, device=self.device),
                torch.full((2, self.E, 7), fill, dtype=torch.float32, device=self.device))

    def poses(self):
        return self.Twc0.clone(), torch.zeros((self.P - 1, 7), dtype=torch.float32, device=self.device)

    def begin(self):
        p = self.m.ptr
        self.m.check(self.L.mslam_gn_begin(p(self.ii), p(self.jj), self.P, self.E, self.HW, *self.wsargs), "gn_begin")

    def compact_at(self, edge_begin, edge_count, slot_begin, range_count, vm=None):
        """The per-edge inputs of [edge_begin, edge_begin + edge_count) as arrays of their own, as a caller with several
        source buffers passes them."""
        p, c = self.m.ptr, self.c
        sl = slice(edge_begin, edge_begin + edge_count)
        idx, v, Q = (a[sl].clone() for a in (self.idx, self.vm if vm is None else vm, self.Q))
        rc = self.L.mslam_gn_compact_at(p(self.Xs), p(self.Cs), p(idx), p(v), p(Q), self.P, self.HW, self.E, edge_begin, edge_count,
                                        slot_begin, range_count, c["C_thresh"], c["Q_thresh"], *self.wsargs)
        self.m.check(rc, "gn_compact_at")
        torch.cuda.synchronize()          # the slices die with this frame

    def compact(self, vm=None):
        p, c = self.m.ptr, self.c
        rc = self.L.mslam_gn_compact(p(self.Xs), p(self.Cs), p(self.idx), p(self.vm if vm is None else vm), p(self.Q), self.P,
                                     self.HW, self.E, 0, self.E, c["C_thresh"], c["Q_thresh"], *self.wsargs)
        self.m.check(rc, "gn_compact")

    def accumulate(self, Twc, Hs, gs):
        p, c = self.m.ptr, self.c
        rc = self.L.mslam_gn_accumulate(KIND[c["kind"]], p(Twc), p(self.K) if c["kind"] == "calib" else 0, self.P, self.HW, self.E,
                                        0, self.E, c["sigma_a"], c["sigma_b"] if c["kind"] != "points" else 1.0, c["h"], c["w"],
                                        c["pixel_border"], c["z_eps"], p(Hs), p(gs), *self.wsargs)
        self.m.check(rc, "gn_accumulate")

    def solve(self, Hs, gs, Twc, dx, delta_thresh=0.0):
        p = self.m.ptr
        rc = self.L.mslam_gn_solve_retract(p(Hs), p(gs), self.P, self.E, self.HW, p(Twc), p(dx), delta_thresh, *self.wsargs)
        self.m.check(rc, "gn_solve_retract")

    def status(self):
        """-> (i32[4], the same 16 bytes as f32[4])."""
        st = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.m.check(self.L.mslam_gn_status(self.m.ptr(st), self.P, self.E, self.HW, *self.wsargs), "gn_status")
        st = st.cpu().numpy().copy()
        return st, st.view(np.float32)

    def blocks(self):
        """begin, compact, one accumulate at the initial poses -> (Hs, gs) as numpy."""
        Hs, gs = self.buffers()
        self.begin()
        self.compact()
        self.accumulate(self.Twc0, Hs, gs)
        return Hs.cpu().numpy(), gs.cpu().numpy()

    def closed(self, max_iter, delta_thresh=0.0, vm=None):
        """mslam_gauss_newton_{rays,calib,points} from the initial poses -> (Twc, dx) tensors."""
        p, c = self.m.ptr, self.c
        Twc, dx = self.poses()
        head = (p(Twc), p(self.Xs), p(self.Cs))
        mid = (p(self.ii), p(self.jj), p(self.idx), p(self.vm if vm is None else vm), p(self.Q), *self.dims)
        tail = (c["C_thresh"], c["Q_thresh"], max_iter, delta_thresh, p(dx), *self.wsargs)
        if c["kind"] == "rays":
            rc = self.L.mslam_gauss_newton_rays(*head, *mid, c["sigma_a"], c["sigma_b"], *tail)
        elif c["kind"] == "calib":
            rc = self.L.mslam_gauss_newton_calib(*head, p(self.K), *mid, c["h"], c["w"], c["pixel_border"], c["z_eps"],
                                                 c["sigma_a"], c["sigma_b"], *tail)
        else:
            rc = self.L.mslam_gauss_newton_points(*head, *mid, c["sigma_a"], *tail)
        self.m.check(rc, "gauss_newton")
        return Twc, dx
