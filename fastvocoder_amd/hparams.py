"""Constants with the reference's names and values (hparams.py:4-24 of the reference): what the
generator path, the mel front end (audio.melspectrogram), Griffin-Lim (audio.inv_mel_spectrogram)
and MODE=preprocess read.  The training
knobs of the reference are out of scope."""
# Mel
num_mels = 80
num_freq = 1025
frame_length_ms = 50
frame_shift_ms = 10
fmin = 40
hop_size = 240
sample_rate = 24000
min_level_db = -100
ref_level_db = 20
preemphasize = True
preemphasis = 0.97
rescale_out = 0.4
signal_normalization = True
# Griffin-Lim (audio.inv_mel_spectrogram)
power = 1.5
griffin_lim_iters = 60

# the index split of MODE=preprocess (bin/preprocess.py)
train_size = 9000
valid_size = 500
eval_size = 100
