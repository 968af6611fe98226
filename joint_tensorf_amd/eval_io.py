"""The files an evaluation leaves behind (model/bat.py:255-259, model/nerf.py:530-556,568-572,619-627): quant_pose.txt, quant.txt
and the PNGs of the rendered views.  Host code on host tensors: nothing here needs a GPU.

quant.txt keeps the reference's four columns `i psnr ssim lpips`.  LPIPS needs trained AlexNet weights that this repository does
not carry: the column holds the values of ops.lpips when the run names the two weight files (eval.lpips.alexnet,
eval.lpips.linear), `nan` otherwise."""
import os
import shutil
import subprocess

import torch

_PIL_WARNED = []


def to_uint8(img):
    """[C, H, W] float in any range -> [H, W, C] uint8: clamp to [0, 1], then torchvision's to_pil_image conversion of float
    tensors (x * 255 truncated to a byte).  The clamp is this build's: the reference does not clamp and wraps around on an
    inverse depth above 1."""
    x = torch.nan_to_num(img.detach().to("cpu", torch.float32), nan=0.0).clamp(0.0, 1.0)   # (0 / 0 of an empty ray: black)
    return x.mul(255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _pil():
    try:
        from PIL import Image
        return Image
    except Exception as e:   # no pictures without it; the numbers are still written
        if not _PIL_WARNED:
            _PIL_WARNED.append(True)
            print("joint_tensorf_amd: PIL cannot be imported (%s): the evaluation PNGs are skipped" % (e,))
        return None


def save_png(img, path):
    """[3, H, W] -> RGB, [1, H, W] -> L (8-bit grey), converted by to_uint8.  Returns False when PIL is missing."""
    Image = _pil()
    if Image is None:
        return False
    a = to_uint8(img).numpy()
    if a.shape[2] == 1:
        Image.fromarray(a[:, :, 0]).save(path)
    elif a.shape[2] == 3:
        Image.fromarray(a).save(path)
    else:
        raise ValueError("save_png: 1 or 3 channels, got %d" % a.shape[2])
    return True


def save_png_bytes(img, path):
    """[H, W, 3] uint8 (a tensor or an array) -> RGB, byte for byte: what a texture atlas is written with.  Returns False when PIL
    is missing."""
    Image = _pil()
    if Image is None:
        return False
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else img
    if a.dtype.name != "uint8" or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("save_png_bytes: uint8 [H, W, 3], got %s %s" % (a.dtype, a.shape))
    Image.fromarray(a).save(path)
    return True


def write_quant_pose(output_path, R_error, t_error):
    """quant_pose.txt: `i err_R err_t` per training view (model/bat.py:255-259)"""
    with open(os.path.join(output_path, "quant_pose.txt"), "w") as f:
        for i, (r, t) in enumerate(zip(R_error, t_error)):
            f.write("{} {} {}\n".format(i, float(r), float(t)))


def write_quant(output_path, psnr_per_view, ssim_per_view, lpips_per_view=None):
    """quant.txt: `i psnr ssim lpips` per held-out view (model/nerf.py:568-572); without `lpips_per_view` the column is nan"""
    if lpips_per_view is None:
        lpips_per_view = [float("nan")] * len(psnr_per_view)
    elif len(lpips_per_view) != len(psnr_per_view):
        raise ValueError("write_quant: %d LPIPS values for %d views" % (len(lpips_per_view), len(psnr_per_view)))
    with open(os.path.join(output_path, "quant.txt"), "w") as f:
        for i, (p, s, l) in enumerate(zip(psnr_per_view, ssim_per_view, lpips_per_view)):
            f.write("{} {} {} {}\n".format(i, float(p), float(s), float(l)))


def write_view_pngs(directory, i, rgb=None, rgb_GT=None, depth=None):
    """<directory>/rgb_<i>.png, rgb_GT_<i>.png, depth_<i>.png (model/nerf.py:554-556, 619-620); maps are [C, H, W]"""
    os.makedirs(directory, exist_ok=True)
    ok = True
    for name, img in (("rgb", rgb), ("rgb_GT", rgb_GT), ("depth", depth)):
        if img is not None:
            ok = save_png(img, os.path.join(directory, "{}_{}.png".format(name, i))) and ok
    return ok


def normalized_invdepth(opt, invdepth_map):
    """model/nerf.py:544-548: NDC inverse depths are mapped from [0.05, far - near] to [0, 1], others are kept"""
    if opt.camera.ndc:
        min_r, max_r = 0.05, opt.nerf.depth.range[1] - opt.nerf.depth.range[0]
        return (invdepth_map - min_r) / (max_r - min_r)
    return invdepth_map


def ndc_render_depth(depth, opacity, center_ndc, ray_ndc, pose, sx, sy, near, tf_near):
    """Camera-axis depth [...] of what a `camera.ndc` render saw, in world units: the render's depth map is batBase.py:148-150's
    sum w t + (1 - opacity) ray_z - tf_near + 0.05 with t the parameter along the NDC ray, so the expected parameter is
    t = (depth + tf_near - 0.05 - (1 - opacity) ray_z) / opacity; the NDC point c + t r (c, r [..., 3]: ops.ray_gen(..., ndc=True)
    of the same pixels) goes through the inverse NDC map (u = 1 - zn, z = 2 near / u, x = xn z / sx, y = yn z / sy) and then
    through the world-to-camera pose [3, 4]: (R p + t)_z.  +inf where the point lies at or behind infinity (u <= 0).  Plain torch
    in the dtype of its arguments, on whatever device they live: a report, not a hot path."""
    t = (depth + tf_near - 0.05 - (1 - opacity) * ray_ndc[..., 2]) / opacity
    p = center_ndc + t[..., None] * ray_ndc
    u = 1 - p[..., 2]
    ok = u > 0
    z = 2 * near / torch.where(ok, u, torch.ones_like(u))
    x, y = p[..., 0] * z / sx, p[..., 1] * z / sy
    d = pose[2, 0] * x + pose[2, 1] * y + pose[2, 2] * z + pose[2, 3]
    return torch.where(ok, d, torch.full_like(d, float("inf")))


def encode_videos(output_path, frame_dir, it=None):
    """The reference's two ffmpeg commands (model/nerf.py:623-627), run only when an ffmpeg executable is on PATH."""
    exe = shutil.which("ffmpeg")
    if exe is None:
        print("joint_tensorf_amd: no ffmpeg on PATH: the frames stay in %s, no video is encoded" % frame_dir)
        return False
    for kind in ("rgb", "depth"):
        out = "{}/novel_view_{}_{}.webm".format(output_path, kind, it)
        subprocess.run([exe, "-y", "-framerate", "30", "-i", "{}/{}_%d.png".format(frame_dir, kind), "-vcodec", "libvpx-vp9",
                        "-pix_fmt", "yuv420p", out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
    return True
