"""`gatys_st` command (mirror of stransfer/clis/gatys_st.py:10-49)."""
import os

import click

from .. import c_logging, constants, img_utils, network

LOGGER = c_logging.get_logger()


def _numbers(value, cast, hint):
    try:
        return [cast(v) for v in value.split(",")]
    except ValueError:
        raise click.BadParameter(f"'{value}': comma-separated numbers expected",
                                 param_hint=hint) from None


def parse_scales(ctx, param, value):
    """--scales 256,512,1024 -> [256, 512, 1024] (scale.check_sizes), or None."""
    if value is None:
        return None
    from .. import scale
    try:
        return scale.check_sizes(_numbers(value, int, "--scales"))
    except ValueError as e:
        raise click.BadParameter(str(e), param_hint="--scales") from None


def parse_scale_steps(ctx, param, value):
    """--scale-steps 300,200,100 -> [300, 200, 100], or None."""
    if value is None:
        return None
    steps = _numbers(value, int, "--scale-steps")
    if min(steps) < 0:
        raise click.BadParameter(f"'{value}': non-negative counts expected",
                                 param_hint="--scale-steps")
    return steps


def level_steps(scales, scale_steps, steps):
    """The per-level step counts: --scale-steps (one per --scales level) or -s at every
    level."""
    if scale_steps is None:
        return steps
    if scales is None:
        raise click.BadParameter("needs --scales", param_hint="--scale-steps")
    if len(scale_steps) != len(scales):
        raise click.BadParameter(f"{len(scale_steps)} counts for the {len(scales)} levels of "
                                 "--scales", param_hint="--scale-steps")
    return scale_steps


def parse_layer_weights(ctx, param, value):
    """--layer-weights a,b,c,d,e -> five floats >= 0, not all zero, or None."""
    if value is None:
        return None
    w = _numbers(value, float, "--layer-weights")
    if len(w) != 5 or min(w) < 0 or not any(w) or any(v != v or v == float("inf") for v in w):
        raise click.BadParameter(f"'{value}': five numbers >= 0, not all zero, expected (one "
                                 "per style tap conv1_1 .. conv3_1)",
                                 param_hint="--layer-weights")
    return w



@click.command()
@click.argument("content-image-path")
@click.argument("style-image-path")
@click.option("-n", "--out-name", default="gatys_converted.png",
              help="The name of the result file (transformed image)")
@click.option("-s", "--steps", default=300,
              help="How many iterations should the optimization go through.")
@click.option("-cw", "--content-weight", default=1,
              help="The weight we will assign to the content loss during the optimization")
@click.option("-sw", "--style-weight", default=100_000,
              help="The weight we will assign to the style loss during the optimization")
@click.option("--optimizer", type=click.Choice(["lbfgs", "adam"]), default="lbfgs",
              help="lbfgs = the reference's train_gatys; adam = one hipGraph replay per iteration")
@click.option("--preserve-color", type=click.Choice(["match", "luminance"]), default=None,
              help="Keep the content image's colours: match = recolour the style image to "
                   "the content's mean and covariance first; luminance = transfer on "
                   "luminance only, then restore the content's chroma")
@click.option("--scales", callback=parse_scales, default=None, metavar="S0,S1,...",
              help="Coarse to fine: transfer at S0, resample the result up and continue at S1, "
                   "... (ascending multiples of 4); the images are loaded at the largest")
@click.option("--scale-steps", callback=parse_scale_steps, default=None, metavar="N0,N1,...",
              help="Iterations per --scales level (default: -s at every level)")
@click.option("--layer-weights", callback=parse_layer_weights, default=None,
              metavar="A,B,C,D,E",
              help="Multipliers of the style weight per style tap, conv1_1 .. conv3_1")
@click.option("--coarse-style", default=None, metavar="PATH",
              help="Mix two styles by scale first: the style image gives the fine scale, PATH "
                   "the coarse scale; the mixed image is the style of the transfer")
@click.option("--fine-taps", type=click.IntRange(1, 4), default=3,
              help="--coarse-style: how many of the five taps count as the fine scale")
@click.option("--mix-steps", type=click.IntRange(min=0), default=None,
              help="--coarse-style: iterations of the mixing transfer (default: -s)")
def gatys_st(content_image_path, style_image_path, out_name, steps, content_weight, style_weight,
             optimizer, preserve_color, scales, scale_steps, layer_weights, coarse_style,
             fine_taps, mix_steps):
    """Run the original Gatys style transfer (slow)."""
    levels = level_steps(scales, scale_steps, steps)
    imsize = None if scales is None else scales[-1]
    root = constants.PROJECT_ROOT_PATH
    style_image = img_utils.image_loader(os.path.join(root, style_image_path), imsize=imsize)
    content_image = img_utils.image_loader(os.path.join(root, content_image_path),
                                           imsize=imsize)
    coarse_image = None if coarse_style is None else \
        img_utils.image_loader(os.path.join(root, coarse_style), imsize=imsize)
    finish = None
    if preserve_color is not None:
        from .. import color  # before StyleNetwork: its Gram targets are taken in __init__
        if coarse_image is None:
            style_image, content_image, finish = color.prepare(style_image, content_image,
                                                               preserve_color)
        else:  # both styles against the same content statistics
            (style_image, coarse_image), content_image, finish = color.prepare(
                [style_image, coarse_image], content_image, preserve_color)
    net = network.StyleNetwork(style_image, content_image)
    if coarse_image is not None:
        from .. import scale
        style_image = scale.mix_scales(net.features(), style_image, coarse_image,
                                       steps if mix_steps is None else mix_steps,
                                       fine_taps=fine_taps, style_weight=style_weight)
        net = network.StyleNetwork(style_image, content_image)
    kw = {} if layer_weights is None else dict(style_layer_weights=layer_weights)
    if scales is not None:
        converted = net.train_gatys_multiscale(style_image, content_image, scales, levels,
                                               optimizer=optimizer, style_weight=style_weight,
                                               content_weight=content_weight, **kw)
    else:
        train = net.train_gatys if optimizer == "lbfgs" else net.train_gatys_adam
        converted = train(style_image=style_image, content_image=content_image,
                          style_weight=style_weight, content_weight=content_weight,
                          steps=steps, **kw)
    if finish is not None:
        converted = finish(converted)
    out_dir = os.path.join(constants.PROJECT_ROOT_PATH, "results")
    os.makedirs(out_dir, exist_ok=True)
    out_file = os.path.join(out_dir, out_name)
    img_utils.imshow(converted, path=out_file)
    LOGGER.info("Done! Transformed image has been saved to: %s", out_file)
