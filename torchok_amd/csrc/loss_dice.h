// The Dice finalize as the two Dice forwards launch it (loss_dice.hip defines it, loss_upsample_dice.hip calls it too).
#pragma once
#include "tok_common.h"

// Folds `nparts` partial rows [3][classes] of (I = sum p y, P = sum p, Y = sum y) into the loss and the two per-class coefficients
// of its gradient, d loss / d p = coef[0][c] y + coef[1][c] (dice_finalize_kernel: smooth, eps, log_loss, the class selection and
// classes without true pixels).  `who` names the entry point in a launch error.
int dice_finalize_launch(const char* who, const float* partial, int nparts, int classes, float smooth, float eps, int log_loss,
                         const int64_t* class_sel, int n_sel, float* loss, float* coef, hipStream_t st);
