"""The two entry points of the reference's src/video_frames_extract.py (:103-121), for the input it reads without a container:
headerless raw YUV (`extract_frames_yuv` / `extract_frames_residual_yuv`, :29-49 and :76-100 - the live_qualcomm dataset).  Where the
reference has ffmpeg write `{video}_{n}.png` and `{video}_{n}_next.png` into sampled_path, these return the clip those files hold:
uint8 BGR [T,2,H,W,3], frame n beside frame n + 1, converted from the file's own bytes (sampling.load_clip_from_yuv on the host,
sampling.GpuYuvLoader with device=...).  Nothing is written; sampled_path is accepted and ignored.

Every other video_type is a container (mp4, mkv, webm): reading it needs a demuxer and an H.264 / HEVC / VP9 decoder, which this
project does not have - those raise.  Decode such files with any decoder to raw frames (or to the PNGs sampling.load_clip_from_frames
reads) first."""
from . import sampling

RAW_VIDEO_TYPES = ("live_qualcomm",)


def container_error(video_type, video_name):
    """What every entry that meets a container raises (data_processing.check_greyscale too)."""
    return NotImplementedError(f"video_type {video_type!r} ({video_name}): container formats need a demuxer and a video decoder; "
                               f"only raw YUV input ({', '.join(RAW_VIDEO_TYPES)}) is read here")


def _clip(video_type, video_name, frame_interval, video_path, video_width, video_height, pixfmt, framerate, device, extended=False):
    if video_type not in RAW_VIDEO_TYPES:
        raise container_error(video_type, video_name)
    if frame_interval is not None and int(frame_interval) != sampling.frame_interval(framerate):
        raise ValueError(f"{video_name}: frame_interval {frame_interval} is not the interval of framerate {framerate} "
                         f"({sampling.frame_interval(framerate)})")
    if device is None:
        return sampling.load_clip_from_yuv(video_path, video_width, video_height, pixfmt, framerate, extended=extended)
    return sampling.GpuYuvLoader([video_path], [video_width], [video_height], [pixfmt], [framerate], device=device, extended=extended)(0)


def process_video_residual(video_type, video_name, frame_interval, video_path, sampled_path, video_width, video_height, pixfmt, framerate,
                           device=None, extended=False):
    """-> uint8 BGR [T,2,H,W,3]: the sampled frames and their successors (a numpy array, or a device tensor with device=...).
    extended=True: pixfmt may be any of sampling.yuv_format's names (10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0, NV21)."""
    return _clip(video_type, video_name, frame_interval, video_path, video_width, video_height, pixfmt, framerate, device, extended)


def process_video(video_type, video_name, frame_interval, video_path, sampled_path, video_width, video_height, pixfmt, framerate,
                  extended=False):
    """-> uint8 BGR [S,H,W,3], a numpy array: every sampled frame (n % interval == 0: the reference's first ffmpeg pass), the last
    one included where it has no successor in the file.  extended: as process_video_residual."""
    if video_type not in RAW_VIDEO_TYPES:
        _clip(video_type, video_name, frame_interval, video_path, video_width, video_height, pixfmt, framerate, None)
    n = sampling.yuv_frame_count(video_path, video_width, video_height, pixfmt, extended)
    sampled, _, _ = sampling.sampled_frame_indices(n, sampling.frame_interval(framerate) if frame_interval is None else frame_interval)
    return sampling.load_frames_from_yuv(video_path, video_width, video_height, pixfmt, sampled, extended=extended)
