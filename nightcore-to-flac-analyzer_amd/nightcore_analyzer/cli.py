"""Command-line interface (same flags, exit codes and JSON as the reference's
cli.py:25-202).

    python -m nightcore_analyzer.cli --nightcore nc.wav --source src.wav -o results.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

from . import pipeline
from .io import ENERGY_GATE_DB, HOP_SEC, SILENCE_STRIP_DB, WINDOW_SEC


def _build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m nightcore_analyzer.cli",
        description=("Extract the precise tempo ratio and pitch ratio between a nightcore track and its "
                     "FLAC source, then emit the Rubber Band parameters needed to reconstruct the original."),
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--nightcore", "-n", required=True, metavar="FILE", help="Nightcore audio file")
    p.add_argument("--source", "-s", required=True, metavar="FILE", help="Source (original) audio file")
    p.add_argument("--output", "-o", metavar="FILE", help="Write JSON results to this file (default: stdout)")
    p.add_argument("--window", type=float, default=WINDOW_SEC, metavar="SEC",
                   help="Analysis window duration in seconds")
    p.add_argument("--hop", type=float, default=HOP_SEC, metavar="SEC",
                   help="Hop between consecutive windows in seconds (< --window for overlap)")
    p.add_argument("--energy-gate", type=float, default=ENERGY_GATE_DB, metavar="DB",
                   help="Discard windows whose RMS energy is below peak + ENERGY_GATE dB")
    p.add_argument("--silence-strip-db", type=float, default=SILENCE_STRIP_DB, metavar="DB",
                   help="Top-dB threshold for trimming leading/trailing silence")
    p.add_argument("--no-silence-strip", action="store_true", help="Disable silence stripping entirely.")
    p.add_argument("--src-trim-sec", type=float, default=0.0, metavar="SEC",
                   help="Manually trim this many seconds from the start of the source")
    p.add_argument("--auto-align", action="store_true", default=False,
                   help="Attempt automatic intro-offset detection (RMS envelope correlation)")
    p.add_argument("--quiet", "-q", action="store_true", help="Suppress progress output")
    p.add_argument("--render-hqnc", metavar="OUT.{wav,flac}", default=None,
                   help="After the analysis, render the source sped up by the detected factor (IBI ratio, "
                        "else tempo ratio) to this file on the GPU: WAV, or FLAC (encoded on the GPU) when "
                        "the name ends in .flac")
    p.add_argument("--refine", action="store_true",
                   help="With --render-hqnc: re-analyse the render against the nightcore and correct the "
                        "factor until the residual is inside tolerance before writing the file")
    p.add_argument("--limit", type=float, nargs="?", const=-0.1, default=None, metavar="DB",
                   help="With --render-hqnc: limit the render to this true-peak ceiling in dBFS on the GPU "
                        "before it is written (-0.1 when no value is given); applies to --pitch-correct too")
    p.add_argument("--pitch-correct", metavar="OUT.{wav,flac}", default=None,
                   help="After the analysis, write the source shifted in pitch by --semitones (duration kept) "
                        "to this file on the GPU: WAV, or FLAC when the name ends in .flac")
    p.add_argument("--semitones", type=float, default=None, metavar="S",
                   help="With --pitch-correct: the shift in semitones (-12 .. 12)")
    p.add_argument("--phase-lock", action="store_true",
                   help="With --pitch-correct: identity phase locking, the file's channels linked to the phases "
                        "of their sum (keeps the level of sustained sounds and the stereo image)")
    return p


def _pitch_correct(args, src_path: Path, log) -> None:
    from . import render
    info = render.pitch_file(src_path, args.pitch_correct, args.semitones, limit_db=args.limit,
                             phase_lock=bool(args.phase_lock))
    if log is not None:
        lock = ", phase-locked" if info.phase_lock else ""
        log(f"\nPitch-corrected file written to: {info.path}  (pitch {info.semitones:+.6f} st{lock}, ratio "
            f"{info.factor:.6f}, peak {info.peak_dbfs:+.2f} dBFS, {info.clipped_samples} clipped samples)")
        if info.limit_db is not None:
            log(f"Limiter at {info.limit_db:+.2f} dBFS: true peak {render._dbfs(info.true_peak):+.2f} dBFS before, "
                f"peak {info.peak_dbfs:+.2f} dBFS after, {info.limited_samples} samples touched")


def _render_hqnc(args, result, nc_path: Path, src_path: Path, log) -> None:
    from . import render
    factor = result.ibi_ratio if result.ibi_ratio is not None else result.tempo_ratio
    if args.refine:
        ref = render.refine_speed(str(nc_path), str(src_path), start=factor, log=log)
        factor = ref.factor
        if log is not None:
            log(f"Refined speed factor: {factor:.6f}× after {ref.corrections} correction(s)"
                + ("" if ref.converged else "  (not converged)"))
    info = render.speed_file(src_path, args.render_hqnc, factor, limit_db=args.limit)
    if log is not None:
        log(f"\nHQNC written to: {info.path}  (speed {info.factor:.6f}×, peak {info.peak_dbfs:+.2f} dBFS, "
            f"{info.clipped_samples} clipped samples)")
        if info.limit_db is not None:
            log(f"Limiter at {info.limit_db:+.2f} dBFS: true peak {render._dbfs(info.true_peak):+.2f} dBFS before, "
                f"peak {info.peak_dbfs:+.2f} dBFS after, {info.limited_samples} samples touched")


def output_dict(result) -> dict:
    """cli.py:171-184 output schema (8-dp rounding; no IBI/xcorr/pitch_method)."""
    return {
        "classification": result.classification,
        "tempo_ratio": round(result.tempo_ratio, 8),
        "pitch_ratio": round(result.pitch_ratio, 8),
        "tempo_ci_95": [round(result.tempo_ci[0], 8), round(result.tempo_ci[1], 8)],
        "pitch_ci_95": [round(result.pitch_ci[0], 8), round(result.pitch_ci[1], 8)],
        "windows_used": {
            "source_pitch": result.n_source_pitch_windows,
            "nightcore_pitch": result.n_nc_pitch_windows,
            "source_tempo": result.n_source_tempo_windows,
            "nightcore_tempo": result.n_nc_tempo_windows,
        },
        "rubberband": result.rubberband,
    }


def main(argv: list[str] | None = None) -> int:
    args = _build_parser().parse_args(argv)
    nc_path, src_path = Path(args.nightcore), Path(args.source)
    errors = []
    if not nc_path.exists():
        errors.append(f"Nightcore file not found: {nc_path}")
    if not src_path.exists():
        errors.append(f"Source file not found:    {src_path}")
    if args.hop >= args.window:
        errors.append("--hop must be less than --window for overlapping windows")
    if args.refine and not args.render_hqnc:
        errors.append("--refine needs --render-hqnc")
    if args.limit is not None and not args.render_hqnc and not args.pitch_correct:
        errors.append("--limit needs --render-hqnc or --pitch-correct")
    if args.pitch_correct and args.semitones is None:
        errors.append("--pitch-correct needs --semitones")
    if args.semitones is not None and not args.pitch_correct:
        errors.append("--semitones needs --pitch-correct")
    if args.phase_lock and not args.pitch_correct:
        errors.append("--phase-lock needs --pitch-correct")
    if args.semitones is not None and not abs(args.semitones) <= 12.0:
        errors.append("--semitones must be within -12 .. 12")
    if args.limit is not None and not args.limit <= 0.0:
        errors.append("--limit must be at or below 0 dBFS")
    if errors:
        for e in errors:
            print(f"ERROR: {e}", file=sys.stderr)
        return 2
    log = None if args.quiet else print
    try:
        result = pipeline.run(str(nc_path), str(src_path), window_sec=args.window, hop_sec=args.hop,
                              energy_gate_db=args.energy_gate,
                              silence_strip_db=None if args.no_silence_strip else args.silence_strip_db,
                              src_trim_sec=args.src_trim_sec,
                              auto_align=args.auto_align and args.src_trim_sec == 0.0, log=log)
    except Exception as exc:
        print(f"\nERROR: {exc}", file=sys.stderr)
        return 1
    text = json.dumps(output_dict(result), indent=2)
    if args.output:
        out = Path(args.output)
        out.write_text(text, encoding="utf-8")
        if not args.quiet:
            print(f"\nResults written to: {out}")
    else:
        print()
        print(text)
    if not args.quiet:
        print()
        print(result)
    if args.render_hqnc:
        try:
            _render_hqnc(args, result, nc_path, src_path, log)
        except Exception as exc:
            print(f"\nERROR: {exc}", file=sys.stderr)
            return 1
    if args.pitch_correct:
        try:
            _pitch_correct(args, src_path, log)
        except Exception as exc:
            print(f"\nERROR: {exc}", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
