"""Mask assembly (yolact_interface.py:678-779, 806-832): score threshold 0.15, masks =
sigmoid(proto @ coef^T) cropped to the box (1 px padding), bilinear to the frame, > 0.5; the 15 best
detections; sum of the masks whose class is 0 (person); (m * 255) as 8 bits (overlaps wrap, as the
reference's `.byte()` does)."""
import torch
import torch.nn.functional as F

SCORE_THRESHOLD = 0.15
TOP_K_DISPLAY = 15
PERSON_CLASS = 0


def _sanitize(a, b, size, padding):
    a, b = a * size, b * size
    lo, hi = torch.min(a, b), torch.max(a, b)
    return torch.clamp(lo - padding, min=0), torch.clamp(hi + padding, max=size)


def _crop(masks, boxes, padding=1):
    """masks [h, w, n]: zero everything outside each detection's (padded) box, box_utils.crop."""
    h, w, n = masks.shape
    x1, x2 = _sanitize(boxes[:, 0], boxes[:, 2], w, padding)
    y1, y2 = _sanitize(boxes[:, 1], boxes[:, 3], h, padding)
    cols = torch.arange(w, device=masks.device, dtype=x1.dtype).view(1, -1, 1)
    rows = torch.arange(h, device=masks.device, dtype=x1.dtype).view(-1, 1, 1)
    inside = (cols >= x1.view(1, 1, -1)) & (cols < x2.view(1, 1, -1)) & (rows >= y1.view(1, 1, -1)) & (rows < y2.view(1, 1, -1))
    return masks * inside.to(masks.dtype)


def postprocess_masks(det, w, h, score_threshold=SCORE_THRESHOLD):
    """Returns (classes, scores, masks[n, h, w] in {0,1}) or None when nothing passes the threshold."""
    if det is None:
        return None
    keep = det["score"] > score_threshold
    if int(keep.sum()) == 0:
        return None
    classes, scores, boxes, coefs = det["class"][keep], det["score"][keep], det["box"][keep], det["mask"][keep]
    masks = torch.sigmoid(det["proto"] @ coefs.t())
    masks = _crop(masks, boxes).permute(2, 0, 1).contiguous()
    masks = F.interpolate(masks.unsqueeze(0), (h, w), mode="bilinear", align_corners=False).squeeze(0)
    return classes, scores, (masks > 0.5).to(torch.float32)


def person_mask(det, w, h):
    """uint8 [h, w] mask, 255 where a person was segmented; None if the network found nothing
    (the reference then raises inside prep_display and the caller's zeroed mask stays in use)."""
    out = postprocess_masks(det, w, h)
    if out is None:
        return None
    classes, scores, masks = out
    order = scores.argsort(0, descending=True)[:TOP_K_DISPLAY]
    classes, masks = classes[order], masks[order]
    total = masks[classes == PERSON_CLASS].sum(0)
    return ((total.to(torch.int64) * 255) & 0xFF).to(torch.uint8)


def person_mask_batch(det, w, h):
    """person_mask for a batch from detect_batch's static-shape output.  Only the (at most 15) detections
    that the reference would display are assembled: the 15 best with score > 0.15, of which the persons
    are summed.  Returns uint8 [B, h, w] and a bool [B] "the network found something" (where it is False
    the reference raises and its caller keeps an all-zero mask)."""
    scores, classes, boxes, coefs, proto = det["score"], det["class"], det["box"], det["mask"], det["proto"]
    B = scores.shape[0]
    valid = scores > SCORE_THRESHOLD
    found = valid.any(dim=1)
    top_scores, order = torch.where(valid, scores, torch.full_like(scores, -1.0)).topk(TOP_K_DISPLAY, dim=1)
    sel_valid = top_scores > SCORE_THRESHOLD
    sel_cls = torch.gather(classes, 1, order)
    sel_box = torch.gather(boxes, 1, order[..., None].expand(-1, -1, 4))
    sel_coef = torch.gather(coefs, 1, order[..., None].expand(-1, -1, coefs.shape[-1]))
    masks = torch.sigmoid(torch.einsum("bhwk,bnk->bnhw", proto, sel_coef))          # [B, 15, 138, 138]
    ph, pw = masks.shape[2:]
    x1, x2 = _sanitize(sel_box[..., 0], sel_box[..., 2], pw, 1)
    y1, y2 = _sanitize(sel_box[..., 1], sel_box[..., 3], ph, 1)
    cols = torch.arange(pw, device=masks.device, dtype=x1.dtype).view(1, 1, 1, -1)
    rows = torch.arange(ph, device=masks.device, dtype=x1.dtype).view(1, 1, -1, 1)
    inside = (cols >= x1[..., None, None]) & (cols < x2[..., None, None]) & (rows >= y1[..., None, None]) & (rows < y2[..., None, None])
    masks = masks * inside.to(masks.dtype)
    person = sel_valid & (sel_cls == PERSON_CLASS)
    if masks.is_cuda and masks.dtype == torch.float32:
        # upsample + threshold + count of the displayed persons + (x 255).byte() in one HIP pass (amos_mask_person_mask_device) instead
        # of a [B, 15, h, w] float tensor and four passes over it
        from .. import mask_person_mask
        masks, flags = masks.contiguous(), person.to(torch.uint8).contiguous()
        out = torch.empty((B, h, w), dtype=torch.uint8, device=masks.device)
        mask_person_mask(torch.cuda.current_stream(masks.device).cuda_stream, masks.data_ptr(), flags.data_ptr(), out.data_ptr(), B, masks.shape[1], ph, pw, h, w)
        return out, found
    masks = F.interpolate(masks, (h, w), mode="bilinear", align_corners=False) > 0.5
    total = (masks & person[..., None, None]).sum(dim=1)
    return ((total.to(torch.int64) * 255) & 0xFF).to(torch.uint8), found


def person_masks_fused(pred, w, h):
    """detect_batch + person_mask_batch as ONE call of this project's library (amos_mask_person_masks_device: seven kernels instead of the
    ~75 small launches the torch ops above cost per pass -- a fifth of a one-frame mask pass): the same selection rules and the same float32
    arithmetic operation by operation, except the 32-term prototype sums (sequential fused multiply-adds here, a BLAS kernel's order there:
    float32 rounding).  Returns (uint8 [B, h, w], bool [B]) like person_mask_batch, or None where it does not apply (not float32 on a
    GPU): the caller then takes the torch path.
    A lazy pass (YolactR50.forward with lazy_coef: no "mask", but "upfeature" and "mask_layer") goes to amos_mask_person_masks_at_priors_device:
    the mask layer is evaluated at the displayed detections' priors, after the selection, from the head's upfeature tensors -- direct float32
    sums where the full pass has the Winograd or library convolution's, so the coefficients agree to float32 rounding of a 2 304-term sum.
    A pass with "candidates" (YolactR50.forward with `candidates`: per-class lists of the scores above SCORE_THRESHOLD instead of "conf" or "cls")
    goes to the _candidates entries: top-k and Fast NMS over the lists, the same masks and `found` bit for bit."""
    ups = pred.get("upfeature")
    loc, coef, priors, proto = pred["loc"], pred.get("mask"), pred["priors"], pred["proto"]
    if ups is not None:
        layer = pred["mask_layer"]
        coef = layer.weight  # (stands in for the dtype checks below)
    cls = pred.get("cls")          # Detect's class scores [B, classes, P] from the head's own kernel (YolactR50.forward(scores_only=True)) ...
    conf = pred.get("conf")        # ... or the softmax tensor [B, P, 1 + classes]
    cand, cand_c1 = pred.get("candidates", (None, None))   # ... or the lists of the scores above SCORE_THRESHOLD (uint8 buffer, classes incl. background)
    scores = cand if cand is not None else cls if cls is not None else conf
    if scores is None or not (loc.is_cuda and all(t.dtype == torch.float32 for t in (loc, coef, priors, proto) + (() if cand is not None else (scores,)))) or proto.dim() != 4:
        return None
    import os
    if os.environ.get("AMOS_MASK_FUSED_POST", "1") == "0":   # A/B runs and the tests that compare the two paths
        return None
    from .. import mask_person_masks, mask_person_masks_scores, mask_post_workspace_bytes
    loc, scores, priors, proto = (t.contiguous() for t in (loc, scores, priors, proto))
    B, P = loc.shape[:2]
    ph, pw, D = proto.shape[1:]
    c1 = cand_c1 if cand is not None else cls.shape[1] + 1 if cls is not None else conf.shape[2]
    if P < 200 or (c1 - 1) * 200 * 4 > 64 * 1024 or D % 4 != 0:
        return None
    nbytes = mask_post_workspace_bytes(B, P, c1, D, ph, pw)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=loc.device)
    out = torch.empty((B, h, w), dtype=torch.uint8, device=loc.device)
    found = torch.empty(B, dtype=torch.uint8, device=loc.device)
    stream = torch.cuda.current_stream(loc.device).cuda_stream
    if ups is not None:
        from .. import mask_person_masks_at_priors
        from .net import Blocked
        weight = layer.weight.contiguous(memory_format=torch.channels_last)  # [anchors x D][3][3][cin] in memory (the engine's layout: no copy)
        anchors = layer.out_channels // D
        if layer.kernel_size != (3, 3) or layer.padding != (1, 1) or layer.stride != (1, 1) or layer.out_channels != anchors * D or layer.bias is None:
            raise RuntimeError("person_masks_fused: the mask layer is not the 3 x 3, padding 1 convolution the lazy pass evaluates")
        blocked = [isinstance(u, Blocked) for u in ups]
        if any(tuple(u.shape[:2]) != (B, layer.in_channels) or u.dtype != torch.float32 for u in ups):
            raise RuntimeError("person_masks_fused: upfeature tensors of another batch, width or type than the pass")
        data = [u.data if f else u for u, f in zip(ups, blocked)]  # held until the call below is enqueued
        if not all(d.is_contiguous() if f else d.is_contiguous(memory_format=torch.channels_last) for d, f in zip(data, blocked)):
            raise RuntimeError("person_masks_fused: an upfeature tensor is neither channels-last nor channel-blocked")
        mask_person_masks_at_priors(stream, loc.data_ptr(), scores.data_ptr(), "candidates" if cand is not None else cls is not None, [d.data_ptr() for d in data], [tuple(u.shape[2:]) for u in ups], blocked,
                                    layer.in_channels, anchors, weight.data_ptr(), layer.bias.data_ptr(), priors.data_ptr(), proto.data_ptr(), B, P, c1, D, ph, pw,
                                    h, w, ws.data_ptr(), nbytes, out.data_ptr(), found.data_ptr())
        return out, found.bool()
    coef = coef.contiguous()
    from .. import mask_person_masks_candidates
    (mask_person_masks_candidates if cand is not None else mask_person_masks_scores if cls is not None else mask_person_masks)(
        stream, loc.data_ptr(), scores.data_ptr(), coef.data_ptr(), priors.data_ptr(), proto.data_ptr(),
        B, P, c1, D, ph, pw, h, w, ws.data_ptr(), nbytes, out.data_ptr(), found.data_ptr())
    return out, found.bool()
