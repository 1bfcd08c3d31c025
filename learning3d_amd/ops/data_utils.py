"""Centring of a cloud pair and its undoing on the estimated transform (reference: ops/data_utils.py:3-45), as PointNetLK's
forward uses them.  Plain torch: a mean over N points and 4x4 products."""
import torch


def _translation(eye3, shift):
    """[B,3,3] identity blocks and a [B,3] shift -> [B,4,4] = [I shift; 0 0 0 1]"""
    top = torch.cat([eye3, shift.unsqueeze(-1)], dim=2)
    bottom = torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).repeat(top.shape[0], 1, 1).to(top)
    return torch.cat([top, bottom], dim=1)


def mean_shift(template, source, p0_zero_mean, p1_zero_mean):
    """-> (template', source', template_mean, source_mean).  A flag that is off leaves its cloud alone and its matrix a [B,3,3]
    identity that postprocess_data never uses.  As in the reference, the SOURCE's matrix carries minus the TEMPLATE's mean
    (ops/data_utils.py:19): results are pinned to that.  p1_zero_mean without p0_zero_mean has no template mean to carry -- the
    reference fails there with a NameError -- and is refused."""
    eye_t = torch.eye(3).view(1, 3, 3).expand(template.size(0), 3, 3).to(template)
    eye_s = torch.eye(3).view(1, 3, 3).expand(source.size(0), 3, 3).to(source)
    template_mean, source_mean = eye_t, eye_s
    if p1_zero_mean and not p0_zero_mean:
        raise ValueError("p1_zero_mean=True needs p0_zero_mean=True (the source's matrix is built from the template's mean)")
    # torch sums a strided cloud (a transposed [B,3,N] buffer) in another order than a dense one: the centre, and behind it every
    # iterate of the loop, would depend on how the caller's tensor lies.  The clouds are made dense first (no copy when they are).
    template, source = template.contiguous(), source.contiguous()
    if p0_zero_mean:
        p0_m = template.mean(dim=1)
        template_mean = _translation(eye_t, p0_m)
        template = template - p0_m.unsqueeze(1)
    if p1_zero_mean:
        p1_m = source.mean(dim=1)
        source_mean = _translation(eye_s, -p0_m)
        source = source - p1_m.unsqueeze(1)
    return template, source, template_mean, source_mean


def postprocess_data(result, p0, p1, a0, a1, p0_zero_mean, p1_zero_mean):
    """est_T <- a0 est_T a1 and the same for every entry of est_T_series [M,B,4,4] (each side only if its flag is on)"""
    est_g = result['est_T']
    est_gs = result['est_T_series']
    if p0_zero_mean:
        est_g = a0.to(est_g).bmm(est_g)
        est_gs = a0.unsqueeze(0).contiguous().to(est_gs).matmul(est_gs)
    if p1_zero_mean:
        est_g = est_g.bmm(a1.to(est_g))
        est_gs = est_gs.matmul(a1.unsqueeze(0).contiguous().to(est_gs))
    result['est_T'] = est_g
    result['est_T_series'] = est_gs
    return result
