"""`python -m stransfer` command groups (mirror of stransfer/clis/__init__.py)."""
import click

from . import adain, fast_st, gatys_guided, gatys_st, gatys_video, video_st


@click.group(commands={
    "video_st": video_st.video_st,
    "fast_st": fast_st.fast_st,
    "gatys_st": gatys_st.gatys_st,
    "gatys_guided": gatys_guided.gatys_guided,
    "gatys_video": gatys_video.gatys_video,
    "adain": adain.adain,
})
def cli():
    """Style Transfer (MI355X)"""
