"""`adain` commands: arbitrary-style transfer (styletransfer_amd/adain.py; no reference
counterpart).  One decoder serves any style image given at conversion time."""
import os

import click

from .. import c_logging, constants
from .fast_st import _loaders

LOGGER = c_logging.get_logger()


@click.group()
def adain():
    """Arbitrary Style Transfer (adaptive instance normalisation)"""


def _style_names(style_paths):
    names = [p.split("/")[-1] for p in style_paths]
    if len(set(names)) != len(names):
        raise click.UsageError(f"style image names must differ: {names}")
    return names


def _weights(mix, style_paths):
    from .. import adain as M
    try:
        return M.parse_style_mix(mix, _style_names(style_paths))
    except ValueError as e:
        raise click.UsageError(str(e))


@adain.command()
@click.argument("style-dir")
@click.option("-n", "--name", required=True, help="Name of the decoder (checkpoint prefix)")
@click.option("-e", "--epochs", default=1, help="How many epochs the training will take")
@click.option("-b", "--batch-size", default=8, help="Batch size for training")
@click.option("-sw", "--style-weight", default=10.0,
              help="The weight of the mean/std style loss")
@click.option("-cw", "--content-weight", default=1.0, help="The weight of the content loss")
@click.option("--lr", default=1e-4, help="Adam's learning rate (decays as 1 / (1 + 5e-5 k))")
@click.option("--seed", default=0, help="Order of the style images; the decoder's initial weights")
@click.option("--synthetic", default=0, type=int,
              help="Train on N synthetic content and style images instead of local COCO and "
                   "STYLE-DIR (no network here)")
@click.option("--gpu-decode", is_flag=True,
              help="COCO loader: workers only Huffman-decode the JPEGs, the IDCT and colour "
                   "conversion run on the GPU (same pixels)")
def train(style_dir, name, epochs, batch_size, style_weight, content_weight, lr, seed, synthetic,
          gpu_decode):
    """Train the AdaIN decoder on the style images under STYLE-DIR (checkpoint per epoch in
    data/models/adain_NAME_epoch*.pth)."""
    from .. import adain as M
    if synthetic:
        styles = M.SyntheticStyles(synthetic, batch_size, seed)
    else:
        styles = M.StyleFolder(os.path.join(constants.PROJECT_ROOT_PATH, style_dir), batch_size,
                               seed)
    LOGGER.info("Training AdaIN decoder %s", name)
    net = M.AdaINNet(decoder_seed=4321 + seed)
    M.train(net, styles, name=name, epochs=epochs,
            loaders=_loaders(batch_size, synthetic, gpu_decode), style_weight=style_weight,
            content_weight=content_weight, lr=lr)


_convert_options = [
    click.option("-n", "--name", required=True, help="Name of the trained decoder"),
    click.option("--alpha", default=1.0, type=click.FloatRange(0.0, 1.0),
                 help="Style strength: 0 keeps the content, 1 is the full transfer"),
    click.option("--mix", default=None,
                 help='Style weights "a.jpg:0.3,b.jpg:0.7" over the given styles (normalised to '
                      "sum 1); default: equal weights"),
    click.option("--preserve-color", is_flag=True,
                 help="Keep the image's colours: only the luminance of the result is used"),
    click.option("-o", "--out-dir", default="results/",
                 help="The results directory where the output will be saved"),
]


def _with(options):
    def deco(f):
        for o in reversed(options):
            f = o(f)
        return f
    return deco


@adain.command()
@click.argument("content")
@click.argument("styles", nargs=-1, required=True)
@_with(_convert_options)
def convert_image(content, styles, name, alpha, mix, preserve_color, out_dir):
    """Convert CONTENT with the style image(s) STYLES through the decoder NAME."""
    from .. import adain as M
    weights = _weights(mix, styles)
    M.AdaINNet().process_image(content, list(styles), mix=weights, alpha=alpha,
                               preserve_color=preserve_color, name=name, out_dir=out_dir)


@adain.command()
@click.argument("clip")
@click.argument("styles", nargs=-1, required=True)
@_with(_convert_options)
@click.option("--fps", default=24.0)
@click.option("--format", "format_", type=click.Choice(["png", "mjpeg"]), default="png",
              help="png = frames in workdir/ (the default); mjpeg = one Motion-JPEG .avi "
                   "written through the GPU JPEG encoder")
@click.option("--quality", default=90, type=click.IntRange(1, 100),
              help="With --format mjpeg: the JPEG quality")
@click.option("--subsampling", type=click.Choice(["444", "422", "420"]), default="420",
              help="With --format mjpeg: the chroma subsampling")
def convert_video(clip, styles, name, alpha, mix, preserve_color, out_dir, fps, format_, quality,
                  subsampling):
    """Convert every frame of CLIP (a Motion-JPEG .avi, a directory of frames or a .npy array)
    with the style image(s) STYLES through the decoder NAME."""
    from .. import adain as M
    weights = _weights(mix, styles)
    out = M.AdaINNet().process_video(clip, list(styles), mix=weights, alpha=alpha,
                                     preserve_color=preserve_color, name=name, out_dir=out_dir,
                                     fps=fps, format=format_, quality=quality,
                                     subsampling=":".join(subsampling))
    click.echo(f"stylised video: {out}")
