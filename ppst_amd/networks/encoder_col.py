"""Colour encoder E2 on HIP kernels (reference: models/networks/encoder_col.py:13-251,
class StyleGAN2ResnetEncodercol).  Trunk = E1's without InstanceNorm; at the four levels
(32@H, 64@H/2, 128@H/4, 256@H/8) cat(GAP, GMP) -> conv1x1 -> 3-layer projector ->
F.normalize gives four (B,2048) codes.  With ``corrmatrix`` the level features are warped
(``warp`` :100-138: pool to 64x64, corr @ feat, bilinear back) before the same heads; the
four corr @ feat products run as ONE fp32-MFMA GEMM over the concatenated 480 channels, so
the 64 MB correspondence matrix is read once instead of four times.  With ``mask`` the
per-class masked heads of :171-245 are produced as well."""
import torch

from .. import ops
from .base_network import BaseNetwork, to_nhwc

TAGS = ["9", "0", "1", "2"]
CH = [32, 64, 128, 256]


class StyleGAN2ResnetEncodercol(BaseNetwork):
    prefix = "E2."

    def _heads(self, jobs):
        """The code heads of several (tag, feature map, mask) jobs.  The jobs do not depend on each other, and each stage of the
        chain -- GAP/GMP, the 1x1 conv, the three projector linears, F.normalize -- is a launch of 8 - 2048 blocks at the batch's
        few rows: every stage runs as ONE grouped launch over the jobs (two for the pooling), each job's values being those of
        its own chain of single calls."""
        if not jobs:
            return []
        tags = [t for t, _, _ in jobs]
        v = [None] * len(jobs)
        for dt in dict.fromkeys(x.dtype for _, x, _ in jobs):     # (one pooling call per storage type)
            idx = [i for i, (_, x, _) in enumerate(jobs) if x.dtype == dt]
            for i, o in zip(idx, ops.gap_gmp_levels([jobs[i][1] for i in idx], [jobs[i][2] for i in idx])):
                v[i] = o
        ws = [self.p("conv1x1_%s.weight" % t) for t in tags]
        v = ops.linear_grouped([(vi, w.reshape(w.shape[0], -1), self.p("conv1x1_%s.bias" % t)) for vi, w, t in zip(v, ws, tags)])
        for layer in ("1", "3", "5"):
            v = ops.linear_grouped([(vi, self.p("projector%s.%s.weight" % (t, layer)), self.p("projector%s.%s.bias" % (t, layer)),
                                     1.0, 1.0, True) for vi, t in zip(v, tags)])
        return ops.l2norm_rows_grouped(v, 1e-12, 1)

    def trunk(self, x, dtype=torch.float32):
        feats = [self.from_rgb_image(x, "FromRGB.", out_dtype=dtype)]
        for i in range(3):
            feats.append(self.res_block(feats[-1], "DownToGlobalCode1.ResBlockDownBy%d." % (2 ** i), ops.PAD_REFLECT, norm=False))
        return feats

    def warp_levels(self, feats, corr):
        """E2.warp for all four levels with one GEMM.  corr (B,4096,4096)."""
        B = feats[0].shape[0]
        V = torch.empty((B, 64, 64, sum(CH)), device=corr.device, dtype=torch.float32)
        off = 0
        for f, c in zip(feats, CH):
            assert f.shape[1] == f.shape[2] and f.shape[1] % 64 == 0, "correspondence needs square inputs (64x64 code grid)"
            ops.avgpool(f, f.shape[1] // 64, out=V[..., off:off + c])
            off += c
        Wv = ops.gemm_nn(corr, V.view(B, 4096, sum(CH)), mode="x3").view(B, 64, 64, sum(CH))
        out, off = [], 0
        for f, c in zip(feats, CH):
            sl = Wv[..., off:off + c]
            out.append(sl if f.shape[1] == 64 else ops.bilinear(sl, f.shape[1], f.shape[2]))
            off += c
        return out

    @staticmethod
    def _mask_planes(mask):
        """NCHW one-hot mask -> list over pyramid levels of (B,H,W,3) NHWC (MaxPool2d(2), :218)."""
        m = to_nhwc(mask)
        if not m.is_contiguous():
            m = m.contiguous()
        levels = [m]
        for _ in range(3):
            levels.append(ops.maxpool2(levels[-1]))
        return levels

    def forward(self, x=None, extract_features=False, mask=None, corrmatrix=None):
        # half-precision activation storage (ops.HALF_STORE) for the plain code pass; the warp / masked heads (pooling,
        # bilinear resize, the correspondence GEMM) read fp32 features
        feats = self.trunk(x, ops.act_dtype() if (corrmatrix is None and mask is None) else torch.float32)
        # every head of the pass -- plain, warped, masked -- goes into the same grouped launches (_heads)
        jobs = [(t, f, None) for t, f in zip(TAGS, feats)]
        warped = None
        if corrmatrix is not None:
            if isinstance(corrmatrix, (list, tuple)):  # simple_swapping_evaluator.py:53 wraps it in a list
                corrmatrix = corrmatrix[0]
            warped = self.warp_levels(feats, corrmatrix.detach())
            jobs += [(t, f, None) for t, f in zip(TAGS, warped)]
        n_w = len(jobs) - 4
        pm_at, pmw_at = [], []
        if mask is not None:
            from .. import glue
            levels = self._mask_planes(mask)
            sw_levels = self._mask_planes(glue.swap(mask)) if warped is not None else None
            for lvl, (t, f) in enumerate(zip(TAGS, feats)):
                for i in range(3):
                    pm_at.append(len(jobs))
                    jobs.append((t, f, levels[lvl][..., i].contiguous()))
                    if warped is not None:
                        pmw_at.append(len(jobs))
                        jobs.append((t, warped[lvl], sw_levels[lvl][..., i].contiguous()))
        out = self._heads(jobs)
        vectors, vectors_w = out[:4], out[4:4 + n_w]
        if mask is not None:
            return vectors, [out[i] for i in pm_at], vectors_w, [out[i] for i in pmw_at]
        return vectors, vectors_w
