"""Hybrid TD3 ensemble driver — counterpart of ``src/all_main/hybrid_td3_main_per.py``.

Same functions (setup_seed, get_model, get_dataset, generate_preds, train, test, submission,
main, eva_stopping) and flags, same files (train_.txt / test_.txt / featindex.txt and the frozen
models' ``{name}best.pth`` in; ``test_prob_weights.csv``, ``test_actions.csv``,
``test_submission.csv``, ``day_aucs.csv``, ``train_rewards.csv`` and the actor's
``actor_modelbest.pth`` out), same semantics: batches in file order, the agent built with
``batch_size=256`` whatever ``--batch_size`` says (line 32), transitions laid out
``[ids | c_actions | d_values | d_action | reward]``, one ``learn`` per batch, ``train`` returning
(last critic loss, reward sum / batches, AUC, learn steps), ``test`` (AUC, mean of the batch BCE
means, reward sum / batches), ``submission`` (predictions, AUC, actions, weights), and the
exploration-rate update of line 330.

Differences, all deliberate:
  * the agent is called with the signatures it has. The reference's ``train`` calls
    ``choose_action(state, exploration_rate)`` and ``store_transition(transitions,
    embedding_layer)``, which ``Hybrid_TD3_model_PER.py`` does not define (it has
    ``choose_action(state)`` and ``store_transition(transitions)``): its loop never runs. The
    exploration rate is computed and kept as in the reference, and not passed to the agent;
  * ``pretrain_main.DeviceBatches`` (slices of one device-resident copy) replaces the eight
    DataLoader workers;
  * ``--metrics host|device`` as in the pretraining drivers, default ``host`` (the reference's
    lists, ``.item()`` per batch and sklearn's AUC). ``device``: every batch goes to a
    ``DeviceMetrics`` accumulator (AUC, loss, rewards), the store is
    ``Hybrid_TD3_Model.store_step`` (one launch, no casts / cat / ones) and ``learn`` returns
    its loss as a tensor, so an epoch of ``train``, and ``test`` and ``submission``, wait for
    the device once, at the final ``compute()``;
  * ``--ensemble_models`` (default ``LR,FM,FFM``, the reference's set, line 294): any names
    ``pretrain_main.build_model`` builds, loaded from ``{save_param_dir}{campaign_id}{name}best.pth``
    and put in ``.eval()`` — the reference's commented-out five-model set (W&D and AFM
    included) is selectable. The state encoder takes its table from ``FMbest.pth`` as in the reference;
  * ids above 2^24: the replay memory stores the ids as fp32 and ``learn`` reads them back with
    ``.long()``, so above 2^24 an id silently becomes another row (latent in the reference);
    ``main`` raises ``ValueError`` when ``feature_nums - 1 > 2**24``;
  * ``train(..., replay=None)``: an iterator of recorded draws, one dict per batch with
    ``act_noise`` (n_c, n_d), ``sample`` (idx, batch, isw) and ``learn_noise`` (n_c, n_d), handed
    to ``choose_action(noise=)`` and ``learn(sample=, noise=)`` (the parity tests); the default
    draws are the agent's own;
  * a missing output directory is created (the reference crashes at its last ``torch.save``).
"""
from __future__ import annotations

import argparse
import datetime
import os

import numpy as np
import pandas as pd
import torch
import torch.nn as nn
from sklearn.metrics import roc_auc_score

from . import creat_data as Data
from . import hip_ops
from . import hybrid_td3_model_per as td3_model
from . import pretrain_main as _pm
from .feature_embedding import Feature_Embedding
from .metrics import DeviceMetrics
from .pretrain_main import DeviceBatches, _check_metrics, eva_stopping, get_dataset, setup_seed

__all__ = ["setup_seed", "get_model", "get_dataset", "generate_preds", "train", "test",
           "submission", "main", "eva_stopping", "load_ensemble"]

MAX_EXACT_ID = 2 ** 24  # the largest id range an fp32 transition column holds exactly


def get_model(action_nums, feature_nums, field_nums, latent_dims, init_lr_a, init_lr_c,
              batch_size, memory_size, device, campaign_id):
    # batch_size=256 whatever the caller passes: hybrid_td3_main_per.py:32
    return td3_model.Hybrid_TD3_Model(feature_nums, field_nums, latent_dims,
                                      action_nums=action_nums, lr_C_A=init_lr_a,
                                      lr_D_A=init_lr_a, lr_C=init_lr_c, campaign_id=campaign_id,
                                      batch_size=256, memory_size=memory_size, device=device)


def generate_preds(model_dict, features, actions, prob_weights, labels, device, mode=None):
    """(y_preds [B,1], rewards [B,1]) of hybrid_td3_main_per.py:56-133: the M frozen models'
    pCTRs, then one kernel (ctr_ensemble_preds_ex: the weights' own softmax, a tie with the
    models' mean rewarded)."""
    M = len(model_dict)
    with torch.no_grad():
        preds = torch.cat([model_dict[i](features).detach().reshape(-1, 1) for i in range(M)],
                          dim=1)
    if labels.is_floating_point():
        labels = labels.long()
    y, r, _ = hip_ops.ensemble_preds_ex(preds, actions, prob_weights, labels, tie_rewards=True,
                                        want_c_actions=False)
    return y, r


def _batches(data_loader):
    """[(features int64 [B,F], labels int64 [B,1], labels float32 [B])]: views of the loader's
    device-resident data, the integer labels converted once for the whole set."""
    if isinstance(data_loader, DeviceBatches):
        x, yf, bs = data_loader.x, data_loader.y, data_loader.batch_size
        yi = yf.long().view(-1, 1)
        return [(x[s:s + bs], yi[s:s + bs], yf[s:s + bs]) for s in range(0, x.shape[0], bs)]
    out = []
    for features, labels in data_loader:
        yi = labels.long().view(-1, 1)
        out.append((features.long(), yi, labels.float().view(-1)))
    return out


def train(rl_model, model_dict, data_loader, embedding_layer, exploration_rate, device,
          metrics="host", replay=None):
    """One epoch (hybrid_td3_main_per.py:136-173)."""
    on_device = _check_metrics(metrics)
    batches = _batches(data_loader)
    if not batches:
        raise ZeroDivisionError("division by zero")  # the reference's empty epoch
    total_critic_loss = 0
    log_intervals = 0
    learn_steps = 0
    total_rewards = 0
    targets, predicts = list(), list()
    acc = DeviceMetrics(sum(int(b[0].shape[0]) for b in batches), batches[0][0].device) \
        if on_device else None

    for features, labels, labels_f in batches:
        draws = next(replay) if replay is not None else {}
        embedding_vectors = embedding_layer.forward(features)
        c_actions, ensemble_c_actions, d_q_values, ensemble_d_actions = rl_model.choose_action(
            embedding_vectors, noise=draws.get("act_noise"))
        y_preds, rewards = generate_preds(model_dict, features, ensemble_d_actions,
                                          ensemble_c_actions, labels, device, mode="train")
        if on_device:
            acc.add(y_preds, labels_f, rewards, with_loss=False)
            rl_model.store_step(features=features, c_actions=c_actions, d_values=d_q_values,
                                d_actions=ensemble_d_actions, rewards=rewards)
        else:
            targets.extend(labels.tolist())
            predicts.extend(y_preds.tolist())
            transitions = torch.cat([features.float(), c_actions, d_q_values,
                                     ensemble_d_actions.float(), rewards], dim=1)
            rl_model.store_transition(transitions)

        total_critic_loss = rl_model.learn(embedding_layer, sample=draws.get("sample"),
                                           noise=draws.get("learn_noise"),
                                           return_tensor=on_device)
        learn_steps += 1
        log_intervals += 1
        if not on_device:
            total_rewards += torch.sum(rewards, dim=0).item()

    if on_device:
        res = acc.compute()  # the epoch's one wait for the device
        return float(total_critic_loss), res["reward_sum"] / log_intervals, res["auc"], learn_steps
    return total_critic_loss, total_rewards / log_intervals, \
        roc_auc_score(targets, predicts), learn_steps


def _evaluate(rl_model, model_dict, embedding_layer, data_loader, device, on_device, loss,
              keep):
    """The loop test() and submission() share (lines 176-225): per batch the greedy action, the
    ensemble and the rewards. Returns (targets, predicts, mean batch loss, reward sum / batches,
    actions, weights, DeviceMetrics result or None)."""
    batches = _batches(data_loader)
    targets, predicts, actions_all, weights_all, ys = [], [], [], [], []
    intervals, total_loss, total_rewards = 0, 0.0, 0.0
    acc = DeviceMetrics(max(sum(int(b[0].shape[0]) for b in batches), 1),
                        batches[0][0].device if batches else device) if on_device else None
    with torch.no_grad():
        for features, labels, labels_f in batches:
            embedding_vectors = embedding_layer.forward(features)
            actions, prob_weights = rl_model.choose_best_action(embedding_vectors)
            y, rewards = generate_preds(model_dict, features, actions, prob_weights, labels,
                                        device, mode="test")
            if on_device:
                acc.add(y, labels_f, rewards)
                if keep:
                    ys.append(y)
            else:
                if loss is not None:
                    total_loss += loss(y, labels.float()).item()
                targets.extend(labels.tolist())
                predicts.extend(y.tolist())
                total_rewards += torch.sum(rewards, dim=0).item()
            if keep:
                actions_all.append(actions)
                weights_all.append(prob_weights)
            intervals += 1
    res = None
    if on_device:
        res = acc.compute()  # the one wait for the device
        total_loss, total_rewards = res["loss"] * intervals, res["reward_sum"]
        if keep:
            predicts = torch.cat(ys).cpu().tolist()
    return targets, predicts, total_loss / intervals, total_rewards / intervals, actions_all, \
        weights_all, res


def test(rl_model, model_dict, embedding_layer, data_loader, loss, device, metrics="host"):
    """(AUC, mean of the batch BCE means, reward sum / batches), lines 176-201."""
    on_device = _check_metrics(metrics)
    targets, predicts, avg_loss, avg_rewards, _, _, res = _evaluate(
        rl_model, model_dict, embedding_layer, data_loader, device, on_device, loss, False)
    auc = res["auc"] if on_device else roc_auc_score(targets, predicts)
    return auc, avg_loss, avg_rewards


def submission(rl_model, model_dict, embedding_layer, data_loader, device, metrics="host"):
    """(predictions, AUC, actions [N,1], prob_weights [N,M]), lines 204-225."""
    on_device = _check_metrics(metrics)
    targets, predicts, _, _, actions, weights, res = _evaluate(
        rl_model, model_dict, embedding_layer, data_loader, device, on_device, None, True)
    auc = res["auc"] if on_device else roc_auc_score(targets, predicts)
    return predicts, auc, torch.cat(actions, dim=0).cpu().numpy(), \
        torch.cat(weights, dim=0).cpu().numpy()


def load_ensemble(names, feature_nums, field_nums, latent_dims, save_param_dir, campaign_id,
                  device):
    """({0: model, ...} in the order of `names`, {name: state_dict}): every frozen model built by
    pretrain_main.build_model, loaded from {save_param_dir}{campaign_id}{name}best.pth, .eval()."""
    model_dict, params = {}, {}
    for i, name in enumerate(names):
        model = _pm.build_model(name, feature_nums, field_nums, latent_dims)
        path = save_param_dir + campaign_id + name + "best.pth"
        params[name] = torch.load(path, map_location="cpu", weights_only=True)
        model.load_state_dict(params[name])
        model.eval()
        model_dict[i] = model.to(device)
    return model_dict, params


def main(data_path, dataset_name, campaign_id, latent_dims, model_name,
         init_lr_a, end_lr_a, init_lr_c, end_lr_c, init_exploration_rate, end_exploration_rate,
         epoch, batch_size, device, save_param_dir, metrics="host",
         ensemble_models=("LR", "FM", "FFM"), memory_size=1000000, verbose=True):
    _check_metrics(metrics)
    if isinstance(ensemble_models, str):
        ensemble_models = [n for n in ensemble_models.split(",") if n]
    if not ensemble_models:
        raise ValueError("ensemble_models: at least one model name")
    os.makedirs(save_param_dir + campaign_id, exist_ok=True)

    device = torch.device(device)
    train_fm, train_data, test_data, field_nums, feature_nums = get_dataset(
        data_path, dataset_name, campaign_id)
    if feature_nums - 1 > MAX_EXACT_ID:
        raise ValueError(
            f"feature_nums = {feature_nums}: the replay memory stores feature ids as float32 and "
            f"learn() reads them back with .long(); ids above 2**24 = {MAX_EXACT_ID} are not "
            "exact in float32 and would silently address another row")

    train_dataset = Data.libsvm_dataset(train_data[:, 1:], train_data[:, 0])
    test_dataset = Data.libsvm_dataset(test_data[:, 1:], test_data[:, 0])
    train_data_loader = DeviceBatches(train_dataset, batch_size, device)
    test_data_loader = DeviceBatches(test_dataset, batch_size, device)

    model_dict, params = load_ensemble(ensemble_models, feature_nums, field_nums, latent_dims,
                                       save_param_dir, campaign_id, device)
    model_dict_len = len(model_dict)

    rl_model = get_model(model_dict_len, feature_nums, field_nums, latent_dims, init_lr_a,
                         init_lr_c, batch_size, memory_size, device, campaign_id)

    embedding_layer = Feature_Embedding(feature_nums, field_nums, latent_dims).to(device)
    fm_params = params.get("FM")
    if fm_params is None:
        fm_params = torch.load(save_param_dir + campaign_id + "FMbest.pth", map_location="cpu",
                               weights_only=True)
    embedding_layer.load_embedding(fm_params)

    loss = nn.BCELoss()
    valid_aucs, valid_losses, history = [], [], []
    start_time = datetime.datetime.now()
    exploration_rate = init_exploration_rate
    rewards_records = []
    global_steps = 0
    for epoch_i in range(epoch):
        train_start_time = datetime.datetime.now()
        train_critic_loss, train_average_rewards, train_auc, learn_steps = train(
            rl_model, model_dict, train_data_loader, embedding_layer, exploration_rate, device,
            metrics=metrics)
        if (epoch_i + 1) % 10 == 0:  # line 330, kept as written
            exploration_rate = max(
                init_exploration_rate - (init_exploration_rate - end_exploration_rate)
                / (epoch - epoch // 10), end_exploration_rate)
        rewards_records.append(train_average_rewards)
        auc, valid_loss, test_rewards = test(rl_model, model_dict, embedding_layer,
                                             test_data_loader, loss, device, metrics=metrics)
        valid_aucs.append(auc)
        valid_losses.append(valid_loss)
        train_end_time = datetime.datetime.now()
        global_steps += learn_steps
        history.append(dict(epoch=epoch_i, critic_loss=train_critic_loss,
                            train_rewards=train_average_rewards, train_auc=train_auc,
                            test_rewards=test_rewards, valid_auc=auc, valid_loss=valid_loss))
        if verbose:
            print("epoch:", epoch_i, "global_steps:", global_steps, "training critic loss:",
                  train_critic_loss, "training average rewards", train_average_rewards,
                  "training auc", train_auc, "test rewards", test_rewards, "validation auc:", auc,
                  "validation loss:", valid_loss,
                  "[{}s]".format((train_end_time - train_start_time).seconds))
    end_time = datetime.datetime.now()

    test_rl_model = rl_model
    auc, test_loss, test_rewards = test(test_rl_model, model_dict, embedding_layer,
                                        test_data_loader, loss, device, metrics=metrics)
    if verbose:
        print("\ntest auc:", auc, datetime.datetime.now(),
              "[{}s]".format((end_time - start_time).seconds))

    submission_path = data_path + dataset_name + campaign_id + model_name + "/"
    os.makedirs(submission_path, exist_ok=True)
    test_predicts, test_auc, actions, prob_weights = submission(
        test_rl_model, model_dict, embedding_layer, test_data_loader, device, metrics=metrics)
    pd.DataFrame(data=prob_weights).to_csv(submission_path + "test_prob_weights.csv", header=None)
    pd.DataFrame(data=actions).to_csv(submission_path + "test_actions.csv", header=None)
    pd.DataFrame(data=test_predicts).to_csv(submission_path + "test_submission.csv", header=None)
    pd.DataFrame(data=[[test_auc]]).to_csv(submission_path + "day_aucs.csv", header=None)
    torch.save(test_rl_model.Hybrid_Actor.state_dict(),
               save_param_dir + campaign_id + "actor_model" + "best.pth")
    pd.DataFrame(data=rewards_records).to_csv(submission_path + "train_rewards.csv", header=None)
    return dict(history=history, test_auc=auc, test_loss=test_loss, test_rewards=test_rewards,
                submission_auc=test_auc, exploration_rate=exploration_rate, agent=test_rl_model)


def _parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_path", default="../../data/")
    parser.add_argument("--dataset_name", default="ipinyou/", help="ipinyou, cretio, yoyi")
    parser.add_argument("--campaign_id", default="1458/", help="1458, 3386")
    parser.add_argument("--model_name", default="Hybrid_TD3_V1",
                        help="the name of the output folder")
    parser.add_argument("--latent_dims", type=int, default=10)
    parser.add_argument("--epoch", type=int, default=300)
    parser.add_argument("--init_lr_a", type=float, default=1e-3)
    parser.add_argument("--end_lr_a", type=float, default=1e-4)
    parser.add_argument("--init_lr_c", type=float, default=1e-3)
    parser.add_argument("--end_lr_c", type=float, default=3e-4)
    parser.add_argument("--init_exploration_rate", type=float, default=1)
    parser.add_argument("--end_exploration_rate", type=float, default=0.1)
    parser.add_argument("--weight_decay", type=float, default=1e-5)
    parser.add_argument("--early_stop_type", default="auc", help="auc, loss")
    parser.add_argument("--batch_size", type=int, default=4096)
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--save_param_dir", default="../models/model_params/")
    parser.add_argument("--metrics", default="host", choices=["host", "device"],
                        help="where AUC, validation loss and rewards are computed")
    parser.add_argument("--ensemble_models", default="LR,FM,FFM",
                        help="comma-separated names pretrain_main.build_model builds: LR, FM, "
                             "FFM, W&D, DeepFM, IPNN, OPNN, FNN, DCN, AFM")
    return parser


if __name__ == "__main__":
    args = _parser().parse_args()
    setup_seed(1)
    main(args.data_path, args.dataset_name, args.campaign_id, args.latent_dims, args.model_name,
         args.init_lr_a, args.end_lr_a, args.init_lr_c, args.end_lr_c,
         args.init_exploration_rate, args.end_exploration_rate, args.epoch, args.batch_size,
         args.device, args.save_param_dir, metrics=args.metrics,
         ensemble_models=args.ensemble_models)
