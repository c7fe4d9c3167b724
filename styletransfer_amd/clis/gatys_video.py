"""`gatys_video` command: temporally consistent Gatys transfer of a clip (Ruder, Dosovitskiy
& Brox 2016, "Artistic Style Transfer for Videos"): every frame is optimised from the
previous result warped along the optical flow, under a consistency-masked temporal loss."""
import os

import click

from .. import c_logging, constants
from .gatys_st import parse_layer_weights

LOGGER = c_logging.get_logger()


def parse_flow(ctx, param, value):
    """--flow static | auto | FLOWS.npz (an existing file under the project root)."""
    if value in ("static", "auto"):
        return value
    path = os.path.join(constants.PROJECT_ROOT_PATH, value)
    if not os.path.isfile(path):
        raise click.BadParameter(f"'{value}': 'static', 'auto' or an .npz file with 'forward' "
                                 "and 'backward' flows expected", param_hint="--flow")
    return path


def parse_long_term(ctx, param, value):
    """--long-term 1,2,4: the offsets of the long-term loss (video.check_offsets)."""
    if value is None:
        return None
    from .. import video
    try:
        return video.check_offsets([int(v) for v in value.split(",")])
    except ValueError as e:
        raise click.BadParameter(str(e), param_hint="--long-term") from None


@click.command()
@click.argument("frames-path")
@click.argument("style-image-path")
@click.option("--flow", required=True, callback=parse_flow, metavar="FLOWS.npz|static|auto",
              help="Optical flows between the conditioned frames: an .npz with 'forward' and "
                   "'backward', each [T-1, 2, S, S] float32 in pixels at the working "
                   "resolution (channel 0 = columns, 1 = rows); static = a fixed camera; "
                   "auto = estimated on the GPU (coarse-to-fine Horn-Schunck)")
@click.option("--save-flows", default=None, metavar="PATH.npz",
              help="With --flow auto: also write the estimated flows to this .npz, which a "
                   "later run takes as --flow")
@click.option("--long-term", callback=parse_long_term, default=None, metavar="1,K,...",
              help="Also tie every frame to the results K frames back, each only where all "
                   "nearer ones are inconsistent (Ruder et al.'s long-term loss): up to 4 "
                   "increasing offsets from 1, e.g. 1,2,4.  A flow file then also holds "
                   "'forward_K' and 'backward_K', each [T-K, 2, S, S]; --save-flows writes them")
@click.option("-s", "--steps", default=100, type=click.IntRange(min=0),
              help="Iterations per frame after the first")
@click.option("--first-steps", default=None, type=click.IntRange(min=0),
              help="Iterations of the first frame (default: -s)")
@click.option("-tw", "--temporal-weight", default=None, type=float,
              help="The weight of the temporal loss (default 200: Ruder et al.'s ratio to a "
                   "content weight of 1)")
@click.option("-cw", "--content-weight", default=1,
              help="The weight we will assign to the content loss during the optimization")
@click.option("-sw", "--style-weight", default=100_000,
              help="The weight we will assign to the style loss during the optimization")
@click.option("--optimizer", type=click.Choice(["adam", "lbfgs"]), default="adam",
              help="adam = one captured engine moved from frame to frame; lbfgs = an L-BFGS "
                   "engine per frame (-s counts its outer steps)")
@click.option("--layer-weights", callback=parse_layer_weights, default=None,
              metavar="A,B,C,D,E",
              help="Multipliers of the style weight per style tap, conv1_1 .. conv3_1")
@click.option("-o", "--out-dir", default="results/gatys_video/",
              help="Where the stylised frames 0.png, 1.png, ... are written")
@click.option("--video", "video_out", default=None, metavar="OUT.avi",
              help="Write the stylised frames as one Motion-JPEG .avi (through the GPU JPEG "
                   "encoder) instead of PNG frames in -o")
@click.option("--fps", default=24.0, help="With --video: the frame rate stored in the file")
@click.option("--quality", default=90, type=click.IntRange(1, 100),
              help="With --video: the JPEG quality")
@click.option("--subsampling", type=click.Choice(["444", "422", "420"]), default="420",
              help="With --video: the chroma subsampling")
def gatys_video(frames_path, style_image_path, flow, save_flows, long_term, steps, first_steps,
                temporal_weight, content_weight, style_weight, optimizer, layer_weights, out_dir,
                video_out, fps, quality, subsampling):
    """Gatys style transfer of a clip, consistent from frame to frame.
    FRAMES_PATH: a directory of frames, a .npy array [T, H, W, 3] uint8 or a Motion-JPEG
    .avi."""
    from .. import img_utils, network, video
    root = constants.PROJECT_ROOT_PATH
    if save_flows is not None and flow != "auto":
        raise click.UsageError("--save-flows needs --flow auto (there is nothing estimated "
                               "to save otherwise)")
    src = os.path.join(root, frames_path)
    frames = list(video.iterate_frames(src))
    if not frames:
        raise click.UsageError(f"no frames in {frames_path}")
    flows = flow
    if save_flows is not None:
        # estimated up front and handed on as explicit flows: the same bits as auto's
        flows = video.estimate_flows(frames, offsets=long_term or (1,))
        if long_term in (None, (1,)):
            video.save_flows(os.path.join(root, save_flows), *flows)
        else:
            video.save_flows(os.path.join(root, save_flows), *flows[1],
                             longer={k: v for k, v in flows.items() if k > 1})
    elif flow not in ("static", "auto"):
        try:
            if long_term is None:
                flows = video.load_flows(flow, len(frames), frames[0].shape[-1])
            else:
                flows = video.load_long_flows(flow, len(frames), frames[0].shape[-1], long_term)
        except ValueError as e:
            raise click.UsageError(str(e)) from None
    style_image = img_utils.image_loader(os.path.join(root, style_image_path))
    net = network.StyleNetwork(style_image)
    out_dir = os.path.join(root, out_dir)
    sink = None
    if video_out is not None:
        video_out = os.path.join(root, video_out)
        os.makedirs(os.path.dirname(video_out) or ".", exist_ok=True)
        sink = video.MjpegSink(video_out, fps, quality, subsampling, constants.DEVICE)
    else:
        os.makedirs(out_dir, exist_ok=True)
    out = net.train_gatys_video(frames, style_image, flows, steps=steps, first_steps=first_steps,
                                temporal_weight=temporal_weight, optimizer=optimizer,
                                style_weight=style_weight, content_weight=content_weight,
                                style_layer_weights=layer_weights, long_term=long_term)
    try:
        for i, y in enumerate(out):
            if sink is not None:
                sink.write(y)
            else:
                img_utils.imshow(y[0], path=os.path.join(out_dir, f"{i}.png"))
    finally:
        if sink is not None:
            sink.close()
    LOGGER.info("Done! %d stylised frames have been saved to: %s", len(frames),
                video_out if sink is not None else out_dir)
