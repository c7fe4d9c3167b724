"""`gatys_guided` command: region-guided Gatys transfer (spatial control of Gatys et al.
2017, "Controlling Perceptual Factors in Neural Style Transfer")."""
import os

import click
import numpy as np
import torch
from PIL import Image

from .. import c_logging, constants, img_utils, network
from .gatys_st import level_steps, parse_scale_steps, parse_scales

LOGGER = c_logging.get_logger()
MAX_REGIONS = 4  # STX_GUIDE_MAX (include/stx.h)


def parse_region(spec: str):
    """STYLE:MASK[:STYLE_MASK] -> (style path, mask path, style mask path or None)."""
    parts = spec.split(":")
    if len(parts) not in (2, 3) or not all(parts):
        raise click.BadParameter(f"'{spec}': expected STYLE:MASK or STYLE:MASK:STYLE_MASK",
                                 param_hint="-r")
    return parts[0], parts[1], parts[2] if len(parts) == 3 else None


def mask_loader(path: str, imsize=None) -> torch.Tensor:
    """A guide as an [H][W] map in [0, 1]: the file read as 8-bit grey, centre-cropped and
    resized as img_utils.image_loader does (no ImageNet normalisation), then / 255."""
    imsize = constants.IMSIZE if imsize is None else imsize
    img = Image.open(path).convert("L")
    img = img_utils._resize(img_utils._center_crop(img, min(img.size)), imsize)
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).float().div(255)


@click.command()
@click.argument("content-image-path")
@click.option("-r", "--region", "regions", multiple=True, required=True,
              metavar="STYLE:MASK[:STYLE_MASK]",
              help="A region: its style image, the mask of the canvas it covers (8-bit "
                   "grey, white = covered) and optionally a mask selecting the part of the "
                   "style image to take the style from.  1 to 4 times.")
@click.option("-n", "--out-name", default="gatys_guided.png",
              help="The name of the result file (transformed image)")
@click.option("-s", "--steps", default=300,
              help="How many iterations should the optimization go through.")
@click.option("-cw", "--content-weight", default=1,
              help="The weight we will assign to the content loss during the optimization")
@click.option("-sw", "--style-weight", default=100_000,
              help="The weight we will assign to the style loss during the optimization")
@click.option("--preserve-color", type=click.Choice(["match", "luminance"]), default=None,
              help="Keep the content image's colours: match = recolour every region's style "
                   "image to the whole content image's mean and covariance first; luminance "
                   "= transfer on luminance only, then restore the content's chroma")
@click.option("--scales", callback=parse_scales, default=None, metavar="S0,S1,...",
              help="Coarse to fine: transfer at S0, resample the result up and continue at S1, "
                   "... (ascending multiples of 4); images and masks are loaded at the largest")
@click.option("--scale-steps", callback=parse_scale_steps, default=None, metavar="N0,N1,...",
              help="Iterations per --scales level (default: -s at every level)")
def gatys_guided(content_image_path, regions, out_name, steps, content_weight, style_weight,
                 preserve_color, scales, scale_steps):
    """Gatys style transfer with one style per masked region of the image."""
    if len(regions) > MAX_REGIONS:
        raise click.UsageError(f"at most {MAX_REGIONS} regions (-r), got {len(regions)}")
    specs = [parse_region(r) for r in regions]
    steps = level_steps(scales, scale_steps, steps)
    top = None if scales is None else scales[-1]
    root = constants.PROJECT_ROOT_PATH
    content_image = img_utils.image_loader(os.path.join(root, content_image_path), imsize=top)
    style_images = [img_utils.image_loader(os.path.join(root, s), imsize=top)
                    for s, _, _ in specs]
    guides = [mask_loader(os.path.join(root, m), top) for _, m, _ in specs]
    style_guides = [None if sm is None else mask_loader(os.path.join(root, sm), top)
                    for _, _, sm in specs]
    if all(g is None for g in style_guides):
        style_guides = None
    finish = None
    if preserve_color is not None:
        from .. import color
        style_images, content_image, finish = color.prepare(style_images, content_image,
                                                            preserve_color)
    net = network.StyleNetwork(style_images[0], content_image)
    converted = net.train_gatys_guided(style_images, content_image, guides,
                                       style_guides=style_guides, style_weight=style_weight,
                                       content_weight=content_weight, steps=steps,
                                       **({} if scales is None else dict(sizes=scales)))
    if finish is not None:
        converted = finish(converted)
    out_dir = os.path.join(root, "results")
    os.makedirs(out_dir, exist_ok=True)
    out_file = os.path.join(out_dir, out_name)
    img_utils.imshow(converted, path=out_file)
    LOGGER.info("Done! Transformed image has been saved to: %s", out_file)
