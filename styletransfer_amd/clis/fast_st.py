"""`fast_st` commands (mirror of stransfer/clis/fast_st.py:11-63)."""
import os

import click
import torch

from .. import c_logging, constants, dataset, img_utils, network

LOGGER = c_logging.get_logger()


@click.group()
def fast_st():
    """Fast Style Transfer"""


def _loaders(batch_size, synthetic, gpu_decode):
    """static_train's `loaders`: None is its default (local COCO, PIL decode in workers)."""
    if synthetic and gpu_decode:
        raise click.UsageError("--gpu-decode applies to the COCO loader, not to --synthetic")
    if synthetic:
        return lambda shard: dataset.get_synthetic_loader(batch_size, n_train=synthetic,
                                                          shard=shard)
    if gpu_decode:
        # static_train's own call, with the switch on
        return lambda shard: dataset.get_coco_loader(test_split=0.10, test_limit=20,
                                                     batch_size=batch_size, shard=shard,
                                                     gpu_decode=True)
    return None


@fast_st.command()
@click.argument("style-image-path")
@click.option("-e", "--epochs", default=50, help="How many epochs the training will take")
@click.option("-b", "--batch-size", default=4, help="Batch size for training")
@click.option("-cw", "--content-weight", default=1,
              help="The weight we will assign to the content loss during the optimization")
@click.option("-sw", "--style-weight", default=100_000,
              help="The weight we will assign to the style loss during the optimization")
@click.option("--synthetic", default=0, type=int,
              help="Train on N synthetic images instead of local COCO (no network here)")
@click.option("--gpu-decode", is_flag=True,
              help="COCO loader: workers only Huffman-decode the JPEGs, the IDCT and colour "
                   "conversion run on the GPU (same pixels)")
def train(style_image_path, epochs, batch_size, content_weight, style_weight, synthetic,
          gpu_decode):
    """Train the fast style transfer network (checkpoint per epoch in data/models/)."""
    from .. import distributed
    distributed.from_env()  # torchrun: one rank per GPU, bound before anything allocates
    style_name = style_image_path.split("/")[-1]
    LOGGER.info("Training fast style transfer network with style name: %s", style_name)
    style_image = img_utils.image_loader(
        os.path.join(constants.PROJECT_ROOT_PATH, style_image_path))
    net = network.ImageTransformNet(style_image, batch_size)
    loaders = _loaders(batch_size, synthetic, gpu_decode)
    net.static_train(style_name=style_name, epochs=epochs, style_weight=style_weight,
                     content_weight=content_weight, loaders=loaders)


@fast_st.command()
@click.argument("style-image-paths", nargs=-1, required=True)
@click.option("-n", "--name", required=True, help="Name of the multi-style network")
@click.option("-e", "--epochs", default=50, help="How many epochs the training will take")
@click.option("-b", "--batch-size", default=4, help="Batch size for training")
@click.option("-cw", "--content-weight", default=1,
              help="The weight we will assign to the content loss during the optimization")
@click.option("-sw", "--style-weight", default=100_000,
              help="The weight we will assign to the style loss during the optimization")
@click.option("--synthetic", default=0, type=int,
              help="Train on N synthetic images instead of local COCO (no network here)")
@click.option("--gpu-decode", is_flag=True,
              help="COCO loader: workers only Huffman-decode the JPEGs, the IDCT and colour "
                   "conversion run on the GPU (same pixels)")
def train_multi(style_image_paths, name, epochs, batch_size, content_weight, style_weight,
                synthetic, gpu_decode):
    """Train ONE network on several styles (conditional instance norm): checkpoints
    data/models/fast_mst_NAME_epoch*.pth and the style names in fast_mst_NAME.styles.json."""
    from .. import distributed
    distributed.from_env()
    names = [p.split("/")[-1] for p in style_image_paths]
    if len(set(names)) != len(names):
        raise click.UsageError(f"style image names must differ: {names}")
    LOGGER.info("Training multi-style network %s on styles: %s", name, names)
    styles = [img_utils.image_loader(os.path.join(constants.PROJECT_ROOT_PATH, p))
              for p in style_image_paths]
    net = network.MultiStyleTransformNet(styles, batch_size, style_names=names)
    loaders = _loaders(batch_size, synthetic, gpu_decode)
    net.static_train(style_name=name, epochs=epochs, style_weight=style_weight,
                     content_weight=content_weight, loaders=loaders)


@fast_st.command()
@click.argument("image-path")
@click.argument("name")
@click.option("--mix", default=None,
              help='Style weights "a.jpg:0.3,b.jpg:0.7" (normalised to sum 1); default: the '
                   "first style")
@click.option("-o", "--out-dir", default="results/",
              help="The results directory where the converted image will be saved")
@click.option("--preserve-color", is_flag=True,
              help="Keep the image's colours: only the luminance of the result is used")
def convert_image_multi(image_path, name, mix, out_dir, preserve_color):
    """Convert IMAGE-PATH with the multi-style network NAME, blending its styles by --mix."""
    try:
        names = network.MultiStyleTransformNet.load_style_names(name)
        weights = network.parse_mix(mix, names)
    except (OSError, ValueError) as e:
        raise click.UsageError(str(e))
    sty = network.MultiStyleTransformNet([torch.rand([3, 8, 8])] * len(names),
                                         style_names=names)
    sty.process_image(image_path=image_path, name=name, mix=weights, out_dir=out_dir,
                      preserve_color=preserve_color)


@fast_st.command()
@click.argument("image-path")
@click.argument("style-name")
@click.option("-o", "--out-dir", default="results/",
              help="The results directory where the converted image will be saved")
@click.option("--preserve-color", is_flag=True,
              help="Keep the image's colours: only the luminance of the result is used")
def convert_image(image_path, style_name, out_dir, preserve_color):
    """Convert IMAGE-PATH with the network pretrained on STYLE-NAME (data/models/)."""
    sty = network.ImageTransformNet(torch.rand([3, 255, 255]))
    sty.process_image(image_path=image_path, style_name=style_name, out_dir=out_dir,
                      preserve_color=preserve_color)
